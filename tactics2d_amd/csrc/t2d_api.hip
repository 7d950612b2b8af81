// t2d_api.hip -- host side of libt2d_hip.so: pool lifetime, uploads, launches (C ABI of
// include/t2d.h).  No CPU compute fallback exists: every entry point that needs the GPU
// returns T2D_ERR_HIP with the HIP error text when the device / runtime is unavailable.
#include <dlfcn.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

// RCCL: types and enums only -- the library is opened with dlopen when a communicator is asked for.  A single-GPU
// install without the rccl development headers still builds: the handful of ABI types used here is declared locally then
// (public NCCL/RCCL ABI: the id is 128 opaque bytes, results and data types are plain enums, ncclUint32 = 3).
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclInt8 = 0, ncclUint8 = 1, ncclInt32 = 2, ncclUint32 = 3 } ncclDataType_t;
}
#endif

#include <algorithm>
#include <functional>
#include <limits>
#include <memory>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "t2d_pool.h"
#include "t2d_host.h"
#include "t2d_step_plan.h"
#ifdef T2D_DEBUG_HOOKS
#include "../../include/t2d_debug.h"
#endif

namespace t2d {
namespace host {
thread_local std::string g_create_err;
int fail(t2d_pool* p, int code, const std::string& msg) {
    if (p) p->err = msg;
    else g_create_err = msg;
    return code;
}
const std::string& create_error() { return g_create_err; }
}  // namespace host
std::atomic<int64_t> g_mem_live[4];
}  // namespace t2d
using namespace t2d::host;
namespace {

// RCCL, opened on demand (t2d_comm_unique_id / t2d_comm_init): libt2d_hip.so itself does not link it, so a single-GPU
// user never loads it, and a process that already holds a copy (torch ships one) shares that copy by soname.
struct Rccl {
    bool tried = false, ok = false;
    std::string err;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    ncclResult_t (*CommCount)(const ncclComm_t, int*) = nullptr;       // optional: t2d_comm_info reads the world back
    ncclResult_t (*CommUserRank)(const ncclComm_t, int*) = nullptr;
};
Rccl& rccl() {
    static Rccl r;
    if (r.tried) return r;
    r.tried = true;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so"})
        if ((h = dlopen(name, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) {
        r.err = std::string("cannot open librccl: ") + dlerror();
        return r;
    }
    r.GetUniqueId = (decltype(r.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    r.CommInitRank = (decltype(r.CommInitRank))dlsym(h, "ncclCommInitRank");
    r.CommDestroy = (decltype(r.CommDestroy))dlsym(h, "ncclCommDestroy");
    r.AllGather = (decltype(r.AllGather))dlsym(h, "ncclAllGather");
    r.GetErrorString = (decltype(r.GetErrorString))dlsym(h, "ncclGetErrorString");
    r.CommCount = (decltype(r.CommCount))dlsym(h, "ncclCommCount");
    r.CommUserRank = (decltype(r.CommUserRank))dlsym(h, "ncclCommUserRank");
    r.ok = r.GetUniqueId && r.CommInitRank && r.CommDestroy && r.AllGather && r.GetErrorString;
    if (!r.ok) r.err = "librccl lacks an expected symbol";
    return r;
}

// Streams the pool has launched on since it was last quiesced.  Set-up calls, up/downloads and t2d_sync wait for
// THESE (plus the pool's own internal streams), not for the device: another pool's env group or a policy running on
// other streams is not stalled by them (no hidden device-wide syncs).
void touch(t2d_pool* p, hipStream_t s) {
    for (int k = 0; k < p->n_live_streams; ++k)
        if (p->live_streams[k] == s) return;
    if (p->n_live_streams < t2d_pool::kMaxLiveStreams) p->live_streams[p->n_live_streams++] = s;
    else p->live_overflow = true;   // more distinct streams than tracked: the next quiesce falls back to the device
}

}  // namespace
namespace t2d { hipError_t launch_chain_rollback(const PoolView& v, const uint32_t* ckpt, hipStream_t s); }
namespace {

hipError_t quiesce(t2d_pool* p) {
    hipError_t e = hipSuccess;
    bool whole_device = p->live_overflow;
    for (int k = 0; k < p->n_live_streams && !whole_device; ++k)
        if (hipStreamSynchronize(p->live_streams[k]) != hipSuccess) {
            // a caller's stream that no longer exists (stepped on a temporary stream and destroyed it): its work cannot be
            // waited for by handle any more -- wait for the device instead of failing or skipping the rest
            (void)hipGetLastError();
            whole_device = true;
        }
    if (whole_device) {
        e = hipDeviceSynchronize();
    } else {   // the pool's own streams, whatever happened above
        if (p->scene_stream) e = hipStreamSynchronize(p->scene_stream);
        if (p->gather_stream) {
            const hipError_t e2 = hipStreamSynchronize(p->gather_stream);
            if (e == hipSuccess) e = e2;
        }
    }
    p->n_live_streams = 0;
    p->live_overflow = false;
    if (e == hipSuccess && p->scene_commit_used && p->scene.commit_err) {
        uint32_t err = 0;
        e = hipMemcpy(&err, p->scene.commit_err, sizeof(err), hipMemcpyDeviceToHost);
        p->scene_commit_used = false;
        if (e == hipSuccess && err) {
            (void)hipMemset(p->scene.commit_err, 0, sizeof(err));
            p->scene_commit_failed = true;
        }
    }
    if (e == hipSuccess && p->trackgen_used && p->trackgen.err) {
        uint32_t err = 0;
        e = hipMemcpy(&err, p->trackgen.err, sizeof(err), hipMemcpyDeviceToHost);
        p->trackgen_used = false;
        if (e == hipSuccess && err) {
            (void)hipMemset(p->trackgen.err, 0, sizeof(err));
            p->trackgen_failed = true;
        }
    }
    if (e == hipSuccess && p->chain_used) {   // a chained launch reports a broken hand-off through two words in device memory
        uint32_t err[2] = {0, 0};   // {1: a bounded wait ran out | 2: producer and consumer on different XCDs, ckpt_tag of the fragment}
        e = hipMemcpy(err, p->d_chain + p->chain_slots, sizeof(err), hipMemcpyDeviceToHost);
        p->chain_used = false;
        if (e == hipSuccess && err[0]) {
            (void)hipMemset(p->d_chain + p->chain_slots, 0, sizeof(err));
            p->chain_failed = true;
            p->chain_err_code = (int)err[0];
            p->chain_steps = false;   // whatever broke the hand-off (a wait that ran out, workgroups of one env set on two XCDs) may do so again
            p->chain_sig = 0;         // (the counters are in no known state: a later chained launch starts them afresh)
            p->chain_rolled_back = false;
            if (p->ckpt_armed && p->d_ckpt) {
                // CHAIN form: whatever the failed fragment and the fragments enqueued behind it computed is discarded -- its
                // checkpoint holds what it started from (complete: its own failure never stops its step-0 stores, a later
                // fragment never overwrites it): put the pool back there.  The tag is the low half of the step count at
                // the fragment's start.
                const uint32_t back = (uint32_t)p->step_count - err[1];
                e = t2d::launch_chain_rollback(p->v, p->d_ckpt, nullptr);
                if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
                if (e == hipSuccess) {
                    p->step_count -= (long long)back;
                    p->chain_rolled_back = true;
                    p->chain_rollback_step = p->step_count;
                    p->v.record = (uint2*)p->field_ptr[T2D_F_RECORD] +
                                  (size_t)((p->step_count + T2D_RECORD_RING - 1) % T2D_RECORD_RING) * p->v.n_env;
                }
            }
        }
    }
    return e;
}

// A failed chained launch is reported ONCE, by the first t2d_sync / t2d_download / t2d_step_n after it; the pool then goes on
// with plain launches (t2d_set_step_chaining turns chaining back on).
int report_chain_failure(t2d_pool* p) {
    if (p->scene_commit_failed) {   // (scene_commit_kernel: cannot happen while the refill cadence below holds)
        p->scene_commit_failed = false;
        return fail(p, T2D_ERR_STATE, "scene regeneration: an env whose episode ended found no staged scene for its next episode and "
                                      "kept its old one -- call t2d_parking_scenes again before stepping on");
    }
    if (p->trackgen_failed) {
        p->trackgen_failed = false;
        return fail(p, T2D_ERR_STATE, "track regeneration: an env's next track came back flagged (the attempt cap, or more tiles than "
                                      "T2D_MAX_TRACK_TILES) and the env kept its old track");
    }
    if (!p->chain_failed) return T2D_OK;
    p->chain_failed = false;
    const std::string why = p->chain_err_code == 2 ? "two workgroups of one env set ran on different XCDs"
                                                   : "a workgroup's bounded wait for its previous step ran out";
    if (p->chain_rolled_back)
        return fail(p, T2D_ERR_STATE, "a t2d_step_n launch failed (" + why + "): the pool was rolled back to step " +
                                          std::to_string(p->chain_rollback_step) + ", the start of the failed fragment -- flags, status, "
                                          "reward and records hold nothing valid until the next step; re-issue the steps from there "
                                          "(they take plain launches now)");
    return fail(p, T2D_ERR_STATE, "a t2d_step_n launch failed (" + why + "): its results are invalid -- t2d_reset / t2d_restore / "
                                      "upload the state before stepping on (plain launches from now on)");
}

size_t field_elem_bytes(int f) {
    switch (f) {
        case T2D_F_RECORD: return 8 * T2D_RECORD_RING;  // ring slots x {u32 reward bits, u32 status word} per env
        case T2D_F_STATUS: return 4;  // 4 x u8 per env
        default: return 4;
    }
}
bool field_per_env(int f) { return f >= T2D_F_ENV_FLAGS && f < T2D_F_LEADER; }

// (Re)initialise the per-env IoU / shaping state: NoAction forgets its pose, _max_iou = -inf,
// _min_dist_to_target = ||start - target centroid|| (envs/parking.py:280-296), inf without targets.
int init_iou_state(t2d_pool* p, const uint8_t* env_mask, const float* hx, const float* hy) {
    const int E = p->v.n_env, A = p->v.A, ego = p->status_cfg.ego_index;
    std::vector<double> maxi(E), mind(E), tc;
    std::vector<uint8_t> lv(E);
    std::vector<int32_t> cna(E);
    std::vector<float> iou(E);
    const bool partial = env_mask != nullptr;
    if (partial) {
        T2D_HIP(p, hipMemcpy(maxi.data(), p->d_max_iou, sizeof(double) * E, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(mind.data(), p->d_min_dist, sizeof(double) * E, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(lv.data(), p->d_last_valid, E, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(cna.data(), p->v.cnt_na, 4 * (size_t)E, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(iou.data(), p->v.iou, 4 * (size_t)E, hipMemcpyDeviceToHost));
    }
    if (p->have_target) {
        tc.resize(2 * (size_t)E);
        T2D_HIP(p, hipMemcpy(tc.data(), p->d_target_c, sizeof(double) * 2 * E, hipMemcpyDeviceToHost));
    }
    for (int e = 0; e < E; ++e) {
        if (partial && !env_mask[e]) continue;
        maxi[e] = -INFINITY;
        lv[e] = 0;
        cna[e] = 0;
        iou[e] = NAN;
        if (p->have_target) {
            const double dx = (double)hx[(size_t)e * A + ego] - tc[2 * (size_t)e];
            const double dy = (double)hy[(size_t)e * A + ego] - tc[2 * (size_t)e + 1];
            mind[e] = sqrt(dx * dx + dy * dy);
        } else {
            mind[e] = INFINITY;
        }
    }
    T2D_HIP(p, hipMemcpy(p->d_max_iou, maxi.data(), sizeof(double) * E, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->d_min_dist, mind.data(), sizeof(double) * E, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->d_last_valid, lv.data(), E, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.cnt_na, cna.data(), 4 * (size_t)E, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.iou, iou.data(), 4 * (size_t)E, hipMemcpyHostToDevice));
    return T2D_OK;
}

// the LDS check of the lidar's edge list: what t2d_lidar_config / t2d_set_static_geometry refuse, both scans refuse too
int lidar_fits(t2d_pool* p) {
    if ((sizeof(double) * (p->lidar.max_slots <= 64 ? 8 : 4) + 8) * (size_t)p->lidar.max_slots + 16 * (size_t)p->lidar.n_beams + 2048 > 60 * 1024)
        return fail(p, T2D_ERR_GEOMETRY, "too many obstacle edges per env for the lidar's LDS edge list");
    return T2D_OK;
}

// plain per-env CSR of the static obstacle rings for the lidar kernel (from the host copy of the geometry)
int rebuild_lidar_geo(t2d_pool* p) {
    if (!p->lidar_on) return T2D_OK;
    const int E = p->v.n_env;
    const auto& g = p->hgeo[0];
    int rc;
    p->lidar.max_static_verts = 0;
    p->lidar.env_vert_cnt = nullptr;
    p->lidar.edge_meta = nullptr;
    if (p->scene_mode) {  // generated scenes: every env owns 4 * T2D_GEN_MAX_QUADS edge slots of d_lidar_xy, the
        constexpr int VS = 4 * T2D_GEN_MAX_QUADS;  // scene kernel maintains the edges and the per-env count
        std::vector<int32_t> evo(E + 1);
        for (int e = 0; e <= E; ++e) evo[e] = VS * e;
        if ((rc = dev_replace(p, &p->d_lidar_env_off, evo.data(), evo.size()))) return rc;
        p->lidar.max_static_verts = VS;
        p->lidar.env_vert_cnt = p->d_lidar_cnt;
        p->lidar.edge_meta = p->d_lidar_meta;   // (ring slots < 16 and <= 48 edges per env by construction)
    } else if (!g.present || g.ring_env_off[E] == 0) {
        if ((rc = dev_replace<int32_t>(p, &p->d_lidar_env_off, nullptr, 0))) return rc;
        if ((rc = dev_replace<float>(p, &p->d_lidar_xy, nullptr, 0))) return rc;
    } else {   // the caller's rings, not the event kernels' fans
        const int P = g.ring_env_off[E], V = g.ring_vert_off[P];
        std::vector<int32_t> evo(E + 1);
        std::vector<float> edges(4 * (size_t)V);   // one record per edge: vertex v and the next vertex of its ring
        for (int e = 0; e <= E; ++e) evo[e] = g.ring_vert_off[g.ring_env_off[e]];
        for (int q = 0; q < P; ++q)
            for (int v = g.ring_vert_off[q]; v < g.ring_vert_off[q + 1]; ++v) {
                const int nx = v + 1 < g.ring_vert_off[q + 1] ? v + 1 : g.ring_vert_off[q];
                edges[4 * (size_t)v] = g.ring_xy[2 * (size_t)v]; edges[4 * (size_t)v + 1] = g.ring_xy[2 * (size_t)v + 1];
                edges[4 * (size_t)v + 2] = g.ring_xy[2 * (size_t)nx]; edges[4 * (size_t)v + 3] = g.ring_xy[2 * (size_t)nx + 1];
            }
        for (int e = 0; e < E; ++e) p->lidar.max_static_verts = std::max(p->lidar.max_static_verts, evo[e + 1] - evo[e]);
        // which rings may take part in the scan's occlusion culling (t2d_lidar.hip): well-shaped rings (the chord bound of
        // the culling argument needs sin(interior angle) >= 0.05 at every vertex) of envs with <= 16 rings and <= 48 edges
        std::vector<uint8_t> meta((size_t)V, 0xff);
        for (int e = 0; e < E; ++e) {
            const int q0 = g.ring_env_off[e], q1 = g.ring_env_off[e + 1];
            if (q1 - q0 > 16 || evo[e + 1] - evo[e] > 48) continue;
            for (int q = q0; q < q1; ++q) {
                const int a = g.ring_vert_off[q], n = g.ring_vert_off[q + 1] - a;
                bool ok = true;
                for (int i = 0; i < n && ok; ++i) {
                    const float* v = &g.ring_xy[2 * (size_t)(a + i)];
                    const float* pr = &g.ring_xy[2 * (size_t)(a + (i + n - 1) % n)];
                    const float* nx = &g.ring_xy[2 * (size_t)(a + (i + 1) % n)];
                    const double ux = (double)pr[0] - v[0], uy = (double)pr[1] - v[1], wx = (double)nx[0] - v[0], wy = (double)nx[1] - v[1];
                    const double cr = std::fabs(ux * wy - uy * wx), den = std::sqrt((ux * ux + uy * uy) * (wx * wx + wy * wy));
                    ok = den > 0.0 && cr >= 0.05 * den;
                }
                if (ok)
                    for (int i = 0; i < n; ++i) meta[(size_t)(a + i)] = (uint8_t)(q - q0);
            }
        }
        if ((rc = dev_replace(p, &p->d_lidar_env_off, evo.data(), evo.size()))) return rc;
        if ((rc = dev_replace(p, &p->d_lidar_xy, edges.data(), edges.size()))) return rc;
        if ((rc = dev_replace(p, &p->d_lidar_meta, meta.data(), meta.size()))) return rc;
        p->lidar.edge_meta = p->d_lidar_meta;
    }
    p->lidar.env_vert_off = p->d_lidar_env_off;
    p->lidar.xy = p->d_lidar_xy;
    p->lidar.max_slots = p->lidar.max_static_verts + (p->lidar.include_participants ? 4 * p->v.A : 0);
    return lidar_fits(p);
}

int record_event(t2d_pool* p, int kernel_id, hipStream_t s, bool begin) {
    if (!p->profiling) return T2D_OK;
    if (begin) {
        if (p->prof_count + 2 > 2 * t2d_pool::kMaxProfSteps) return T2D_OK;  // buffer full
    } else if (!(p->prof_count & 1)) {
        return T2D_OK;  // the matching begin was skipped
    }
    T2D_HIP(p, hipEventRecord(p->prof_events[p->prof_count], s));
    p->prof_kernel[p->prof_count] = kernel_id;
    p->prof_count++;
    return T2D_OK;
}

// What t2d_curve_routes, t2d_spline_routes, t2d_planview_routes and t2d_polyline_routes ask after their family's own argument check, and the bracket
// around their launch: count_dev and route are arguments, the installed route sets state (route_slot in t2d_route_write_dev.h
// relies on it).  launch(s) is the family's launch_*_routes line under T2D_HIP, so that a launch error names the call.
template <class Launch>
int write_routes(t2d_pool* p, const std::string& who, int profile_id, int32_t route, const int32_t* count_dev, void* hip_stream,
                 Launch launch) {
    if (reinterpret_cast<uintptr_t>(count_dev) & 3u) return fail(p, T2D_ERR_INVALID, who + ": misaligned count_dev");
    if (route < 0) return fail(p, T2D_ERR_INVALID, who + ": route must be >= 0");
    if (p->route.kind != 1) return fail(p, T2D_ERR_STATE, who + " writes into route sets: t2d_set_routes must precede it");
    if (!p->route_sets_distinct)
        return fail(p, T2D_ERR_STATE, who + ": two envs share a route set; install one set per env (set_of_env)");
    if (route >= p->route_min_limit)
        return fail(p, T2D_ERR_STATE, who + ": route " + std::to_string(route) + " does not exist in every env's set (the smallest set has " +
                                          std::to_string(p->route_min_limit) + " routes)");
    hipStream_t s = (hipStream_t)hip_stream;
    T2D_HIP(p, hipSetDevice(p->device));
    touch(p, s);
    int rc;
    if ((rc = record_event(p, profile_id, s, true))) return rc;
    if ((rc = launch(s))) return rc;
    return record_event(p, profile_id, s, false);
}

}  // namespace


namespace t2d {
namespace {
struct SnapPtrs { const float* f[6]; const uint32_t* ids; };
__global__ __launch_bounds__(256) void restore_kernel(PoolView pv, SnapPtrs sp, int mode) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= pv.N) return;
    const int env = i / pv.A;
    if (mode == 1) {
        const uchar4 st = reinterpret_cast<const uchar4*>(pv.status)[env];
        if (!(st.z | st.w)) return;
    }
    pv.x[i] = sp.f[0][i]; pv.y[i] = sp.f[1][i]; pv.heading[i] = sp.f[2][i];
    pv.speed[i] = sp.f[3][i]; pv.vx[i] = sp.f[4][i]; pv.vy[i] = sp.f[5][i];
    pv.ids[i] = sp.ids[i];
    pv.flags[i] = 0;
    pv.applied0[i] = 0.f; pv.applied1[i] = 0.f;   // nothing applied yet in the new episode (State.accel of a reset)
    if (pv.snap_omega[0]) {
        pv.omega_f[i] = pv.snap_omega[0][i];
        pv.omega_r[i] = pv.snap_omega[1][i];
    }
    // the env record (status, counters) is cleared by restore_env_kernel, launched after this
    // kernel on the same stream, so every participant has read `status` before it changes
}
// one wave that does nothing for `ticks` of the 100 MHz real-time counter (t2d_debug_delay_gather)
__global__ __launch_bounds__(64) void spin_kernel(long long ticks) {
    const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
    while ((long long)(__builtin_amdgcn_s_memrealtime() - t0) < ticks) __builtin_amdgcn_s_sleep(32);
}
__global__ __launch_bounds__(256) void restore_env_kernel(PoolView pv, int mode) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= pv.n_env) return;
    if (mode == 1) {
        const uchar4 st = reinterpret_cast<const uchar4*>(pv.status)[env];
        if (!(st.z | st.w)) return;
    }
    pv.env_flags[env] = 0; pv.cnt_step[env] = 0; pv.frame_ms[env] = 0; pv.reward[env] = 0.f;
    pv.last_valid[env] = 0; pv.cnt_na[env] = 0; pv.max_iou[env] = -INFINITY;
    pv.min_dist[env] = pv.snap_min_dist[env]; pv.iou[env] = NAN;
    uchar4 st; st.x = T2D_SCENARIO_NORMAL; st.y = T2D_TRAFFIC_NORMAL; st.z = 0; st.w = 0;
    reinterpret_cast<uchar4*>(pv.status)[env] = st;
}
// back to the checkpoint of a failed CHAIN fragment (PoolView::ckpt): the state arrays and the envs' counters
__global__ __launch_bounds__(256) void chain_rollback_kernel(PoolView pv, const uint32_t* ck) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const size_t n = (size_t)pv.N;
    if (i < pv.N) {
        // (every slot of the pool was loaded and checkpointed by the fragment's first step, active or not; a point mass's
        // velocity is the only velocity that is state)
        const uint32_t ids = ck[6 * n + i];
        pv.x[i] = __uint_as_float(ck[i]);
        pv.y[i] = __uint_as_float(ck[n + i]);
        pv.heading[i] = __uint_as_float(ck[2 * n + i]);
        pv.speed[i] = __uint_as_float(ck[3 * n + i]);
        if (((ids >> kIdsActiveShift) & 0xffu) && ((ids >> kIdsModelShift) & 0xffu) == T2D_MODEL_POINTMASS) {
            pv.vx[i] = __uint_as_float(ck[4 * n + i]);
            pv.vy[i] = __uint_as_float(ck[5 * n + i]);
        }
        pv.ids[i] = ids;
    }
    if (i < pv.n_env) {
        pv.cnt_step[i] = (int32_t)ck[7 * n + i];
        pv.frame_ms[i] = (int32_t)ck[7 * n + pv.n_env + i];
    }
}
}  // namespace
void pool_touch(t2d_pool* p, hipStream_t s) { touch(p, s); }
hipError_t launch_chain_rollback(const PoolView& v, const uint32_t* ckpt, hipStream_t s) {
    hipLaunchKernelGGL(chain_rollback_kernel, dim3((v.N + 255) / 256), dim3(256), 0, s, v, ckpt);
    return hipGetLastError();
}
hipError_t launch_spin(long long ticks, hipStream_t s) {
    hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, s, ticks);
    return hipGetLastError();
}
hipError_t launch_restore(const PoolView& v, const float* const* snap, const uint32_t* snap_ids, int mode,
                          hipStream_t s) {
    SnapPtrs sp;
    for (int k = 0; k < 6; ++k) sp.f[k] = snap[k];
    sp.ids = snap_ids;
    hipLaunchKernelGGL(restore_kernel, dim3((v.N + 255) / 256), dim3(256), 0, s, v, sp, mode);
    hipLaunchKernelGGL(restore_env_kernel, dim3((v.n_env + 255) / 256), dim3(256), 0, s, v, mode);
    return hipGetLastError();
}
}  // namespace t2d

extern "C" {

static void refresh_idm_view(t2d_pool* p);

const char* t2d_last_error(const t2d_pool* pool) {
    return pool ? pool->err.c_str() : create_error().c_str();
}
int t2d_abi_version(void) { return T2D_ABI_VERSION; }

int t2d_create(int32_t n_env, int32_t max_agents, int32_t device_id, t2d_pool** out_pool) {
    if (!out_pool) return fail(nullptr, T2D_ERR_INVALID, "out_pool is null");
    *out_pool = nullptr;
    if (n_env <= 0 || max_agents <= 0 || max_agents > T2D_MAX_AGENTS)
        return fail(nullptr, T2D_ERR_INVALID, "n_env must be > 0 and 1 <= max_agents <= 256");
    if ((int64_t)n_env * max_agents > (int64_t)1 << 30)
        return fail(nullptr, T2D_ERR_INVALID, "pool too large");
    int n_dev = 0;
    T2D_HIP(nullptr, hipGetDeviceCount(&n_dev));
    if (device_id < 0 || device_id >= n_dev)
        return fail(nullptr, T2D_ERR_HIP, "HIP device " + std::to_string(device_id) + " not available (" +
                                              std::to_string(n_dev) + " devices visible)");
    T2D_HIP(nullptr, hipSetDevice(device_id));
    t2d_pool* p = new (std::nothrow) t2d_pool();
    if (!p) return fail(nullptr, T2D_ERR_NOMEM, "host allocation failed");
    p->device = device_id;
    // (read once, here; 0 where the query fails: such a pool takes no form that counts on resident workgroups)
    (void)hipDeviceGetAttribute(&p->device_cus, hipDeviceAttributeMultiprocessorCount, device_id);
    p->v.n_env = n_env;
    p->v.A = max_agents;
    p->v.N = n_env * max_agents;
    for (int f = 0; f < T2D_F_COUNT; ++f) {
        const size_t n = field_per_env(f) ? (size_t)n_env : (size_t)p->v.N;
        p->field_bytes[f] = n * field_elem_bytes(f);
        if (f == T2D_F_LIDAR) {  // sized by t2d_lidar_config
            p->field_bytes[f] = 0;
            continue;
        }
        const hipError_t e = p->field_buf[f].alloc_zeroed(p->field_bytes[f]);
        p->field_ptr[f] = p->field_buf[f];
        if (e != hipSuccess) {
            std::string msg = std::string("hipMalloc/hipMemset: ") + hipGetErrorString(e);
            t2d_destroy(p);
            return fail(nullptr, e == hipErrorOutOfMemory ? T2D_ERR_NOMEM : T2D_ERR_HIP, msg);
        }
    }
    hipError_t e = p->d_params.alloc(T2D_PARAM_COLS * T2D_MAX_TYPES);
    if (e != hipSuccess) {
        t2d_destroy(p);
        return fail(nullptr, T2D_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    {
        const size_t E = (size_t)n_env;
        p->chain_slots = (n_env + 7 + 8) & ~7;   // one counter per step workgroup (at most one per env) + padding; then the error word
        hipError_t e2 = p->d_last_pose.alloc_zeroed(E * 8);
        if (e2 == hipSuccess) e2 = p->d_max_iou.alloc_zeroed(E);
        if (e2 == hipSuccess) e2 = p->d_min_dist.alloc_zeroed(E);
        if (e2 == hipSuccess) e2 = p->d_snap_min_dist.alloc_zeroed(E);
        if (e2 == hipSuccess) e2 = p->d_last_valid.alloc_zeroed(E);
        if (e2 == hipSuccess) e2 = p->d_chain.alloc_zeroed((size_t)p->chain_slots + 1);
        if (e2 != hipSuccess) {
            t2d_destroy(p);
            return fail(nullptr, T2D_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(e2));
        }
    }
    t2d::PoolView& v = p->v;
    v.x = (float*)p->field_ptr[T2D_F_X];
    v.y = (float*)p->field_ptr[T2D_F_Y];
    v.heading = (float*)p->field_ptr[T2D_F_HEADING];
    v.speed = (float*)p->field_ptr[T2D_F_SPEED];
    v.vx = (float*)p->field_ptr[T2D_F_VX];
    v.vy = (float*)p->field_ptr[T2D_F_VY];
    v.act0 = (float*)p->field_ptr[T2D_F_ACT0];
    v.act1 = (float*)p->field_ptr[T2D_F_ACT1];
    v.act_stride = 1;
    v.applied0 = (float*)p->field_ptr[T2D_F_APPLIED0];
    v.applied1 = (float*)p->field_ptr[T2D_F_APPLIED1];
    v.out_mask = (int32_t)T2D_OUT_ALL;
    v.omega_f = (float*)p->field_ptr[T2D_F_OMEGA_F];
    v.omega_r = (float*)p->field_ptr[T2D_F_OMEGA_R];
    v.ids = (uint32_t*)p->field_ptr[T2D_F_IDS];
    v.flags = (uint32_t*)p->field_ptr[T2D_F_FLAGS];
    v.env_flags = (uint32_t*)p->field_ptr[T2D_F_ENV_FLAGS];
    v.cnt_step = (int32_t*)p->field_ptr[T2D_F_CNT_STEP];
    v.frame_ms = (int32_t*)p->field_ptr[T2D_F_FRAME_MS];
    v.status = (uint8_t*)p->field_ptr[T2D_F_STATUS];
    v.reward = (float*)p->field_ptr[T2D_F_REWARD];
    v.record = (uint2*)p->field_ptr[T2D_F_RECORD];
    v.iou = (float*)p->field_ptr[T2D_F_IOU];
    v.cnt_na = (int32_t*)p->field_ptr[T2D_F_CNT_NO_ACTION];
    v.target_xy = nullptr;
    v.target_c = nullptr;
    v.last_pose = p->d_last_pose;
    v.last_valid = p->d_last_valid;
    v.max_iou = p->d_max_iou;
    v.min_dist = p->d_min_dist;
    v.snap_min_dist = p->d_snap_min_dist;
    v.params = p->d_params;
    v.cell = 1.0;
    v.inv_cell = 1.0;
    v.dbg = nullptr;
    v.map_flags = nullptr;
    for (int k = 0; k < 6; ++k) v.snap[k] = nullptr;
    v.snap_ids = nullptr;
    v.auto_reset = 0;
    v.overlapped = 0;
    v.wgmap = nullptr;
#ifdef T2D_TIMING
    {   // (T2D_TIMING_WORDS: room for the chained form's record per wave AND step, scripts/chain_timing.py)
        size_t words = (size_t)(n_env + 64) * 16 * 4;
        if (const char* e = getenv("T2D_TIMING_WORDS")) words = std::max(words, (size_t)strtoull(e, nullptr, 10));
        (void)p->d_dbg.alloc_zeroed(words);
        v.dbg = p->d_dbg;
    }
#endif
    v.geo = nullptr;
    v.geo_layout = t2d::GeoLayout{};
    p->v.n_env = n_env;   // (envs_per_workgroup reads it)
    v.geo_layout.epb = envs_per_workgroup(p, log2_pad(max_agents));
    // ParkingEnv defaults: envs/parking.py:106 (max_step 2e4), :151-163 (reward table)
    p->status_cfg = t2d_status_config{20000, 0, 0, 0, -5.0f, -1.0f, -5.0f, 5.0f, 0.001f,
                                      0, 0, 100, 0, 0.95f, 0.999f, 0.1f};
#ifndef T2D_CHAIN_DEPTH_DEFAULT
#define T2D_CHAIN_DEPTH_DEFAULT 1
#endif
    p->chain_depth = T2D_CHAIN_DEPTH_DEFAULT;
#ifdef T2D_EXPERIMENTS   // (builds with -DT2D_EXPERIMENTS carry the instantiation; the product's depth is 1)
    if (const char* e = getenv("T2D_CHAIN_DEPTH")) p->chain_depth = std::max(1, std::min(16, atoi(e)));
#endif
    *out_pool = p;
    return T2D_OK;
}

static void unbind_trajectories(t2d_pool* p);   // (defined with struct t2d_traj)

int t2d_destroy(t2d_pool* p) {
    if (!p) return T2D_OK;
    (void)hipSetDevice(p->device);
    (void)quiesce(p);  // nothing of this pool may still be running (incl. a scene refill on its own stream)
    unbind_trajectories(p);
    if (p->comm && rccl().ok) (void)rccl().CommDestroy((ncclComm_t)p->comm);
    if (p->gather_stream) (void)hipStreamDestroy(p->gather_stream);
    if (p->ev_frag_ready) (void)hipEventDestroy(p->ev_frag_ready);
    for (hipEvent_t e : p->ev_gather)
        if (e) (void)hipEventDestroy(e);
    if (p->scene_stream) (void)hipStreamDestroy(p->scene_stream);
    if (p->ev_scene_commit) (void)hipEventDestroy(p->ev_scene_commit);
    if (p->ev_scene_refill) (void)hipEventDestroy(p->ev_scene_refill);
    if (p->prof_events) {
        for (int i = 0; i < 2 * t2d_pool::kMaxProfSteps; ++i) (void)hipEventDestroy(p->prof_events[i]);
        delete[] p->prof_events;
    }
    delete p;   // (every buffer: the members free themselves)
    return T2D_OK;
}

int t2d_set_param_table(t2d_pool* p, const double* rows, int32_t n_types, int32_t row_stride) {
    if (!p) return T2D_ERR_INVALID;
    if (!rows || n_types <= 0 || n_types > T2D_MAX_TYPES || row_stride < T2D_PARAM_COLS)
        return fail(p, T2D_ERR_INVALID, "need 1..32 types and row_stride >= 24");
    T2D_HIP(p, hipSetDevice(p->device));
    std::vector<double> t(T2D_PARAM_COLS * T2D_MAX_TYPES, 0.0);
    double dmax = 0.0;
    bool has_drift = false;
    uint32_t replay_types = 0u;
    for (int ty = 0; ty < n_types; ++ty) {
        const double* r = rows + (size_t)ty * row_stride;
        const int model = (int)r[T2D_P_MODEL];
        if (model < 0 || model > T2D_MODEL_REPLAY)
            return fail(p, T2D_ERR_INVALID, "row " + std::to_string(ty) + ": unknown model id");
        const bool replayed = model == T2D_MODEL_REPLAY;   // (shape, length and width only: no range, mass or sub-step column is read)
        if (replayed) replay_types |= 1u << ty;
        if (model == T2D_MODEL_POINTMASS_EULER) has_drift = true;   // (integrated by the side kernel, like the drift model)
        if (model == T2D_MODEL_DRIFT) {
            has_drift = true;
            if (!(r[T2D_P_MASS] > 0.0) || !(r[T2D_P_IZ] > 0.0) || !(r[T2D_P_DRIFT_RADIUS] > 0.0) ||
                !(r[T2D_P_DRIFT_IYW] > 0.0) || !(r[T2D_P_LF] != 0.0))
                return fail(p, T2D_ERR_INVALID, "row " + std::to_string(ty) +
                                                    ": SingleTrackDrift needs mass, I_z, radius, I_yw > 0 and lf != 0");
        }
        const int dt = (int)r[T2D_P_DELTA_T_MS];
        if (dt < 1 && !replayed) return fail(p, T2D_ERR_INVALID, "row " + std::to_string(ty) + ": delta_t must be >= 1 ms");
        if (model != T2D_MODEL_POINTMASS && model != T2D_MODEL_POINTMASS_EULER && !replayed && !(r[T2D_P_WB] != 0.0))
            return fail(p, T2D_ERR_INVALID, "row " + std::to_string(ty) + ": zero wheel base");
        for (int c = 0; c < T2D_PARAM_COLS; ++c) {
            p->host_params[ty][c] = r[c];
            t[(size_t)c * T2D_MAX_TYPES + ty] = r[c];
        }
        const double L = r[T2D_P_LENGTH], W = r[T2D_P_WIDTH];
        const double br = (int)r[T2D_P_SHAPE] == T2D_SHAPE_CIRCLE ? 0.5 * W : 0.5 * sqrt(L * L + W * W);
        t[(size_t)T2D_P_RESERVED0 * T2D_MAX_TYPES + ty] = br;  // bounding radius for the reject test
        // (a replayed row's delta_t is never used, but the derive launch divides by every row's: keep the device's copy >= 1)
        if (replayed && dt < 1) t[(size_t)T2D_P_DELTA_T_MS * T2D_MAX_TYPES + ty] = 1.0;
        if (model != T2D_MODEL_DRIFT) {   // the two derived columns (include/t2d.h): the sub-step in seconds now, its counts per launch interval
            t[(size_t)T2D_P_DT_S * T2D_MAX_TYPES + ty] = (double)dt / 1000;
            t[(size_t)T2D_P_SUBSTEPS * T2D_MAX_TYPES + ty] = 0.0;
        }
        dmax = std::max(dmax, 2.0 * br);
    }
    p->v.n_types = n_types;
    p->has_drift = has_drift;
    p->replay_types = replay_types;
    p->all_boxes = true;
    for (int ty = 0; ty < n_types; ++ty)
        if ((int)p->host_params[ty][T2D_P_SHAPE] != T2D_SHAPE_OBB) p->all_boxes = false;
    p->v.cell = dmax * 1.001 + 1e-3;  // 3x3 cell neighbourhood is then provably sufficient
    p->v.inv_cell = 1.0 / p->v.cell;
    T2D_HIP(p, quiesce(p));
    T2D_HIP(p, hipMemcpy(p->d_params, t.data(), sizeof(double) * t.size(), hipMemcpyHostToDevice));
    // the derived column (T2D_P_SUBSTEPS) of the new table, for the interval the pool was last stepped with, at once: a
    // captured graph of step launches does not hold the derive launch and would otherwise replay on a column of zeros
    // (no sub-steps at all, silently) after a new table
    const int prev_interval = p->derived_interval;
    p->derived_interval = -1;   // (the next stepping call derives again: the host-side values travel with it)
    if (prev_interval > 0) {
        T2D_HIP(p, t2d::launch_derive(p->d_params, n_types, prev_interval, nullptr));
        T2D_HIP(p, hipStreamSynchronize(nullptr));
    }
    p->have_params = true;
    return T2D_OK;
}

int t2d_set_static_geometry(t2d_pool* p, const int32_t* env_poly_offsets,
                            const int32_t* poly_vert_offsets, const float* verts_xy,
                            const float* boundary, const uint8_t* boundary_valid) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    ++p->geo_gen;
    const int E = p->v.n_env;
    int rc;
    if (p->scene_mode) {  // host-described geometry replaces the generated scenes
        p->scene_mode = p->scene_regen = false;
        if ((rc = dev_replace<float>(p, &p->d_lidar_xy, nullptr, 0))) return rc;
    }
    if (env_poly_offsets) {
        if (!poly_vert_offsets || (!verts_xy && env_poly_offsets[E] > 0))
            return fail(p, T2D_ERR_INVALID, "polygon CSR arrays missing");
        if ((rc = prepare_polys(p, env_poly_offsets, poly_vert_offsets, verts_xy, p->hgeo[0])) != T2D_OK)
            return rc;
    } else {
        p->hgeo[0] = t2d_pool::HostGeo{};
    }
    if ((rc = rebuild_geo(p)) != T2D_OK) return rc;
    if ((rc = rebuild_lidar_geo(p)) != T2D_OK) return rc;
    if (boundary) {
        if ((rc = dev_replace(p, &p->d_boundary, boundary, (size_t)4 * E))) return rc;
        if ((rc = dev_replace(p, &p->d_boundary_valid, boundary_valid, boundary_valid ? (size_t)E : 0)))
            return rc;
    } else {
        if ((rc = dev_replace<float>(p, &p->d_boundary, nullptr, 0))) return rc;
        if ((rc = dev_replace<uint8_t>(p, &p->d_boundary_valid, nullptr, 0))) return rc;
    }
    p->v.boundary = p->d_boundary;
    p->v.boundary_valid = p->d_boundary_valid;
    return T2D_OK;
}

int t2d_set_lane_geometry(t2d_pool* p, const int32_t* env_lane_offsets,
                          const int32_t* lane_vert_offsets, const float* verts_xy) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    ++p->geo_gen;
    const int E = p->v.n_env;
    int rc;
    if (p->scene_mode) return fail(p, T2D_ERR_STATE, "lane geometry cannot be combined with generated parking scenes");
    if (env_lane_offsets) {
        if (!lane_vert_offsets || (!verts_xy && env_lane_offsets[E] > 0))
            return fail(p, T2D_ERR_INVALID, "lane CSR arrays missing");
        if ((rc = prepare_polys(p, env_lane_offsets, lane_vert_offsets, verts_xy, p->hgeo[1])) != T2D_OK)
            return rc;
        build_lane_boundary(E, p->hgeo[1]);
        build_safe_rects(E, p->hgeo[1]);
    } else {
        p->hgeo[1] = t2d_pool::HostGeo{};
    }
    return rebuild_geo(p);
}

int t2d_set_target_areas(t2d_pool* p, const float* target_xy, const float* centroid) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    const int E = p->v.n_env;
    int rc;
    if (p->scene_mode) return fail(p, T2D_ERR_STATE, "target areas belong to the generated parking scenes; "
                                                      "call t2d_set_static_geometry first to leave that mode");
    if (!target_xy) {
        if ((rc = dev_replace<double>(p, &p->d_target_xy, nullptr, 0))) return rc;
        if ((rc = dev_replace<double>(p, &p->d_target_c, nullptr, 0))) return rc;
        p->have_target = false;
    } else {
        std::vector<double> xy(8 * (size_t)E), c(2 * (size_t)E);
        for (int e = 0; e < E; ++e) {
            std::vector<double> q(8);
            for (int k = 0; k < 8; ++k) q[k] = (double)target_xy[8 * (size_t)e + k];
            double a = area2(q);
            if (a < 0.0) {  // clockwise -> reverse
                for (int i = 0, j = 3; i < j; ++i, --j) {
                    std::swap(q[2 * i], q[2 * j]);
                    std::swap(q[2 * i + 1], q[2 * j + 1]);
                }
                a = -a;
            }
            if (!(a > 0.0)) return fail(p, T2D_ERR_GEOMETRY, "target area " + std::to_string(e) + " is degenerate");
            for (int i = 0; i < 4; ++i)
                if (orient_h(&q[2 * i], &q[2 * ((i + 1) & 3)], &q[2 * ((i + 2) & 3)]) < 0.0)
                    return fail(p, T2D_ERR_GEOMETRY, "target area " + std::to_string(e) + " is not convex");
            memcpy(&xy[8 * (size_t)e], q.data(), 8 * sizeof(double));
            if (centroid) {
                c[2 * (size_t)e] = centroid[2 * (size_t)e];
                c[2 * (size_t)e + 1] = centroid[2 * (size_t)e + 1];
            } else {  // area centroid of the polygon (shapely Polygon.centroid)
                double cx = 0.0, cy = 0.0;
                for (int i = 0; i < 4; ++i) {
                    const int j = (i + 1) & 3;
                    const double w = q[2 * i] * q[2 * j + 1] - q[2 * j] * q[2 * i + 1];
                    cx += (q[2 * i] + q[2 * j]) * w;
                    cy += (q[2 * i + 1] + q[2 * j + 1]) * w;
                }
                c[2 * (size_t)e] = cx / (3.0 * a);
                c[2 * (size_t)e + 1] = cy / (3.0 * a);
            }
        }
        if ((rc = dev_replace(p, &p->d_target_xy, xy.data(), xy.size()))) return rc;
        if ((rc = dev_replace(p, &p->d_target_c, c.data(), c.size()))) return rc;
        p->have_target = true;
    }
    p->v.target_xy = p->d_target_xy;
    p->v.target_c = p->d_target_c;
    if (p->have_reset) {  // distance-to-target of the shaping restarts from the current state
        const size_t N = (size_t)p->v.N;
        std::vector<float> hx(N), hy(N);
        T2D_HIP(p, hipMemcpy(hx.data(), p->v.x, 4 * N, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hy.data(), p->v.y, 4 * N, hipMemcpyDeviceToHost));
        if ((rc = init_iou_state(p, nullptr, hx.data(), hy.data()))) return rc;
    }
    return T2D_OK;
}

int t2d_set_status_config(t2d_pool* p, const t2d_status_config* cfg) {
    if (!p) return T2D_ERR_INVALID;
    if (!cfg) return fail(p, T2D_ERR_INVALID, "cfg is null");
    if (cfg->ego_index < 0 || cfg->ego_index >= p->v.A)
        return fail(p, T2D_ERR_INVALID, "ego_index out of range");
    p->status_cfg = *cfg;
    // time-penalty term of ParkingEnv._get_reward (envs/parking.py:156-158) for every possible step count: the
    // epilogue then reads one double instead of evaluating tanh on one lane at the very end of the wave
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    std::vector<double> tp;
    if (cfg->max_step > 0 && cfg->max_step <= (1 << 24)) {
        tp.resize((size_t)cfg->max_step + 1);
        for (int c = 0; c <= cfg->max_step; ++c)
            tp[c] = -tanh((double)c / (double)cfg->max_step) * (double)cfg->time_penalty_scale;
    }
    int rc = dev_replace(p, &p->d_time_penalty, tp.data(), tp.size());
    if (rc != T2D_OK) return rc;
    p->v.time_penalty = p->d_time_penalty;
    return T2D_OK;
}

int t2d_reset(t2d_pool* p, const uint8_t* env_mask, const float* x, const float* y,
              const float* heading, const float* speed, const float* vx, const float* vy,
              const uint8_t* type_id, const uint8_t* active) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->have_params) return fail(p, T2D_ERR_STATE, "t2d_set_param_table must precede t2d_reset");
    if (!x || !y || !heading || !speed || !type_id || !active)
        return fail(p, T2D_ERR_INVALID, "x, y, heading, speed, type_id, active are required");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    if (!env_mask) p->chain_failed = false;   // (every env gets a new state: whatever a failed t2d_step_n left behind is gone)
    const int E = p->v.n_env, A = p->v.A, N = p->v.N;
    std::vector<float> hx(N), hy(N), hh(N), hs(N), hvx(N), hvy(N);
    std::vector<uint32_t> hids(N), hflags(N);
    std::vector<uint32_t> henv(E);
    std::vector<int32_t> hcnt(E), hframe(E);
    std::vector<uint8_t> hstat(4 * (size_t)E);
    std::vector<float> hrew(E);
    const bool partial = env_mask != nullptr;
    if (partial) {  // read-modify-write of the unselected envs
        T2D_HIP(p, hipMemcpy(hx.data(), p->v.x, 4 * (size_t)N, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hy.data(), p->v.y, 4 * (size_t)N, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hh.data(), p->v.heading, 4 * (size_t)N, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hs.data(), p->v.speed, 4 * (size_t)N, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hvx.data(), p->v.vx, 4 * (size_t)N, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hvy.data(), p->v.vy, 4 * (size_t)N, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hids.data(), p->v.ids, 4 * (size_t)N, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hflags.data(), p->v.flags, 4 * (size_t)N, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(henv.data(), p->v.env_flags, 4 * (size_t)E, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hcnt.data(), p->v.cnt_step, 4 * (size_t)E, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hframe.data(), p->v.frame_ms, 4 * (size_t)E, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hstat.data(), p->v.status, 4 * (size_t)E, hipMemcpyDeviceToHost));
        T2D_HIP(p, hipMemcpy(hrew.data(), p->v.reward, 4 * (size_t)E, hipMemcpyDeviceToHost));
    }
    uint32_t types_used = partial ? p->types_used : 0u;   // (T2D_MAX_TYPES = 32 rows: one bit each)
    for (int e = 0; e < E; ++e) {
        if (partial && !env_mask[e]) continue;
        for (int a = 0; a < A; ++a) {
            const size_t i = (size_t)e * A + a;
            const int ty = type_id[i];
            if (active[i] && ty >= p->v.n_types)
                return fail(p, T2D_ERR_INVALID, "type_id " + std::to_string(ty) + " not in the parameter table");
            hx[i] = x[i]; hy[i] = y[i]; hh[i] = heading[i]; hs[i] = speed[i];
            if (vx && vy) {
                hvx[i] = vx[i]; hvy[i] = vy[i];
            } else {  // State.velocity: (speed*cos(heading), speed*sin(heading))  state.py:161-166
                hvx[i] = (float)((double)speed[i] * cos((double)heading[i]));
                hvy[i] = (float)((double)speed[i] * sin((double)heading[i]));
            }
            const int model = active[i] ? (int)p->host_params[ty][T2D_P_MODEL] : 0;
            if (active[i]) types_used |= 1u << ty;
            hids[i] = ((uint32_t)model << t2d::kIdsModelShift) | ((uint32_t)ty << t2d::kIdsTypeShift) |
                      ((uint32_t)(active[i] ? 1 : 0) << t2d::kIdsActiveShift);
            hflags[i] = 0;
        }
        henv[e] = 0; hcnt[e] = 0; hframe[e] = 0; hrew[e] = 0.0f;
        hstat[4 * (size_t)e] = T2D_SCENARIO_NORMAL; hstat[4 * (size_t)e + 1] = T2D_TRAFFIC_NORMAL;
        hstat[4 * (size_t)e + 2] = 0; hstat[4 * (size_t)e + 3] = 0;
    }
    T2D_HIP(p, hipMemcpy(p->v.x, hx.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.y, hy.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.heading, hh.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.speed, hs.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.vx, hvx.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.vy, hvy.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.ids, hids.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.flags, hflags.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.env_flags, henv.data(), 4 * (size_t)E, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.cnt_step, hcnt.data(), 4 * (size_t)E, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.frame_ms, hframe.data(), 4 * (size_t)E, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.status, hstat.data(), 4 * (size_t)E, hipMemcpyHostToDevice));
    T2D_HIP(p, hipMemcpy(p->v.reward, hrew.data(), 4 * (size_t)E, hipMemcpyHostToDevice));
    {  // SingleTrackDrift wheel speeds start at rest (the reference's callers pass omega = 0 for a new episode), and nothing
       // has been applied yet: T2D_F_APPLIED0 / 1 are 0.0 (what the cruise / ACC law reads as accel_last)
        std::vector<float> ho(N, 0.0f);
        for (int f : {T2D_F_OMEGA_F, T2D_F_OMEGA_R, T2D_F_APPLIED0, T2D_F_APPLIED1}) {
            if (partial) {
                T2D_HIP(p, hipMemcpy(ho.data(), p->field_ptr[f], 4 * (size_t)N, hipMemcpyDeviceToHost));
                for (int e = 0; e < E; ++e)
                    if (env_mask[e]) std::fill(ho.begin() + (size_t)e * A, ho.begin() + (size_t)(e + 1) * A, 0.0f);
            }
            T2D_HIP(p, hipMemcpy(p->field_ptr[f], ho.data(), 4 * (size_t)N, hipMemcpyHostToDevice));
        }
    }
    {
        int rc2 = init_iou_state(p, env_mask, hx.data(), hy.data());
        if (rc2 != T2D_OK) return rc2;
    }
    // (an armed auto-reset may put the snapshot's ids back into any env from the next step on)
    p->types_used = types_used | (p->auto_reset ? p->snap_types : 0u);
    p->have_reset = true;
    if (!partial && p->pid.on) {   // new episodes everywhere: controller.reset()
        const int rc = t2d_pid_reset(p, nullptr, nullptr);
        if (rc != T2D_OK) return rc;
    }
    if (!partial && p->rs_follow_on) return t2d_rs_follow_reset(p, nullptr, nullptr);   // new episodes everywhere: agent.reset()
    return T2D_OK;
}

// IDM lanes read the pool's own action fields; only while caller-owned actions are bound do the kernels need to tell
// the two apart
static void refresh_idm_view(t2d_pool* p) {
    const bool bound = p->v.act0 != (const float*)p->field_ptr[T2D_F_ACT0];
    const bool sel = p->idm.on && bound;
    p->v.idm_ctrl = sel ? p->idm.d_ctrl : nullptr;
    p->v.own_act0 = sel ? (const float*)p->field_ptr[T2D_F_ACT0] : nullptr;
    p->v.own_act1 = sel ? (const float*)p->field_ptr[T2D_F_ACT1] : nullptr;
}

int t2d_bind_actions_strided(t2d_pool* p, const float* act0_dev, const float* act1_dev, int32_t stride) {
    if (!p) return T2D_ERR_INVALID;
    if ((act0_dev == nullptr) != (act1_dev == nullptr))
        return fail(p, T2D_ERR_INVALID, "bind both action arrays or neither");
    if (act0_dev && stride < 1) return fail(p, T2D_ERR_INVALID, "action stride must be >= 1 element");
    p->v.act0 = act0_dev ? act0_dev : (const float*)p->field_ptr[T2D_F_ACT0];
    p->v.act1 = act1_dev ? act1_dev : (const float*)p->field_ptr[T2D_F_ACT1];
    p->v.act_stride = act0_dev ? stride : 1;
    p->act_in_frame = false;
    p->act_extent = 0;   // how far the new memory reaches is not known until the caller says (t2d_set_action_extent)
    refresh_idm_view(p);
    return T2D_OK;
}

int t2d_set_action_extent(t2d_pool* p, int64_t n_elements) {
    if (!p) return T2D_ERR_INVALID;
    if (n_elements < 0) return fail(p, T2D_ERR_INVALID, "the action extent is a number of elements (0 = not declared)");
    if (n_elements && p->v.act0 == (const float*)p->field_ptr[T2D_F_ACT0])
        return fail(p, T2D_ERR_STATE, "t2d_set_action_extent describes memory bound with t2d_bind_actions[_strided]");
    if (n_elements && (int64_t)(p->v.N - 1) * p->v.act_stride >= n_elements)
        return fail(p, T2D_ERR_INVALID, "the declared extent does not hold one action per participant at the bound stride");
    p->act_extent = n_elements;
    return T2D_OK;
}

int t2d_bind_actions(t2d_pool* p, const float* act0_dev, const float* act1_dev) {
    return t2d_bind_actions_strided(p, act0_dev, act1_dev, 1);
}

static int drift_impl(t2d_pool* p, int interval_ms, hipStream_t s) {
    int rc;
    touch(p, s);
    if ((rc = record_event(p, 5, s, true))) return rc;
    T2D_HIP(p, t2d::launch_drift(p->v, interval_ms, s));
    return record_event(p, 5, s, false);
}

static int idm_impl(t2d_pool* p, hipStream_t s, const int32_t* forced_leader = nullptr) {
    int rc;
    touch(p, s);
    if ((rc = record_event(p, 4, s, true))) return rc;
    T2D_HIP(p, t2d::launch_idm(p->v, p->idm.view, forced_leader, (float*)p->field_ptr[T2D_F_ACT0],
                               (float*)p->field_ptr[T2D_F_ACT1], s));
    return record_event(p, 4, s, false);
}

// what a stepping launch needs of its interval beside the integer: interval_ms / 1000 (PointMass's dt) in the view, and the
// sub-step counts per type in the device table (one 32-thread launch on the step's stream whenever the interval changes)
// Coefficients of the resummed kinematic step (PoolView::kin_coef) for n sub-steps.  With u = k - m the centred sub-step
// index, w = u / M, the step's Euler sum  sum_k v_k (cos, sin)(theta_k),  theta_k = Theta + a w + b w^2,  v_k = V + ah M w,
// needs the means over k of cos / sin / w cos / w sin of (a w + b w^2); expanding in a (to a^(2 D + 1)) and b (to b^3) and
// using that the odd moments of w vanish leaves eight polynomials in a^2 whose coefficients are moments mu_p = mean(w^p)
// over factorials (SingleTrackKinematics._step, physics/single_track_kinematics.py:126-176, is the sum being restated).
static void kinematics_resum_table(t2d::PoolView& v, int n) {
    v.kin_n = 0;
    if (n < 1) return;
    constexpr int D = t2d::kKinDegree;
    const long double m = ((long double)n - 1) / 2, M = (long double)n / 2;
    long double mu[2 * D + 9];
    for (int q = 0; q <= 2 * D + 8; ++q) mu[q] = 0;
    for (int k = 0; k < n; ++k) {
        const long double w = ((long double)k - m) / M;
        long double pw = 1;
        for (int q = 0; q <= 2 * D + 8; ++q) {
            mu[q] += pw;
            pw *= w;
        }
    }
    for (int q = 0; q <= 2 * D + 8; ++q) mu[q] /= (long double)n;
    long double fact[2 * D + 3];
    fact[0] = 1;
    for (int q = 1; q <= 2 * D + 2; ++q) fact[q] = fact[q - 1] * q;
    for (int i = 0; i <= D; ++i) {
        const long double sg = (i & 1) ? -1.0L : 1.0L;
        const long double qe = sg / fact[2 * i], ro = sg / fact[2 * i + 1];
        v.kin_coef[i][t2d::KIN_Q0] = (double)(qe * mu[2 * i]);                  // E cos:   Q0 + b^2 Q4
        v.kin_coef[i][t2d::KIN_Q4] = (double)(-0.5L * qe * mu[2 * i + 4]);
        v.kin_coef[i][t2d::KIN_Q2] = (double)(qe * mu[2 * i + 2]);              // E sin:   b (Q2 + b^2 Q6)
        v.kin_coef[i][t2d::KIN_Q6] = (double)(-qe * mu[2 * i + 6] / 6);
        v.kin_coef[i][t2d::KIN_R4] = (double)(-ro * mu[2 * i + 4]);             // E w cos: a b (R4 + b^2 R8)
        v.kin_coef[i][t2d::KIN_R8] = (double)(ro * mu[2 * i + 8] / 6);
        v.kin_coef[i][t2d::KIN_R2] = (double)(ro * mu[2 * i + 2]);              // E w sin: a (R2 + b^2 R6)
        v.kin_coef[i][t2d::KIN_R6] = (double)(-0.5L * ro * mu[2 * i + 6]);
    }
    const double g[8] = {(double)m, (double)M, (double)(m - 0.5L), (double)(m * (m - 1) / 2), (double)(M * M / 2),
                         (double)(m + 1), (double)((m + 1) * (m + 1) / 2), (double)n};
    memcpy(v.kin_geo, g, sizeof g);
    v.kin_n = n;
}

static int prepare_interval(t2d_pool* p, int interval_ms, hipStream_t s) {
    if (interval_ms > T2D_MAX_INTERVAL_MS) return fail(p, T2D_ERR_INVALID, "interval_ms must be <= 32767");
    p->v.interval_s = (double)interval_ms / 1000;
    if (p->derived_interval != interval_ms) {
        // the resummed kinematic step is built for ONE sub-step count: that of the first SingleTrackKinematics row (every
        // type shares delta_t = 5 ms unless a caller says otherwise); lanes of a type with another count take the loop
        int kn = 0;
        for (int t = 0; t < p->v.n_types && !kn; ++t)
            if ((int)p->host_params[t][T2D_P_MODEL] == T2D_MODEL_KINEMATICS && p->host_params[t][T2D_P_DELTA_T_MS] >= 1.0)
                kn = interval_ms / (int)p->host_params[t][T2D_P_DELTA_T_MS];
        // ... and only pools that put at least two waves on every SIMD: a lone wave is a latency chain, and the table's scalar
        // loads (cache misses on first touch) lengthen it by more than the twenty loop trips they replace (same-box A/B,
        // 512 x 32 envs one launch per step: 12.8 -> 13.4 us with the series)
        const bool fills = (long long)p->v.N >= 2LL * 64 * 4 * (p->device_cus > 0 ? p->device_cus : 256);
        kinematics_resum_table(p->v, p->kin_resum && (fills || p->kin_resum_forced) ? kn : 0);
        touch(p, s);
        T2D_HIP(p, t2d::launch_derive(p->d_params, p->v.n_types, interval_ms, s));
        p->derived_interval = interval_ms;
    }
    return T2D_OK;
}

// Replayed participants (T2D_MODEL_REPLAY rows): pools that hold one keep helper launches around the step, as pools with a drift
// row do -- no single-ego kernel, no chained form, controllers in a launch of their own
static bool side_models(const t2d_pool* p) { return p->has_drift || p->replay_types != 0u; }

// what plan_step (t2d_step_plan.h) decides the form of the pool's step launch from.  t2d_step fills it on every call: plain reads,
// no allocation, no walk over a vector
static StepFacts step_facts(const t2d_pool* p) {
    StepFacts f{};
    f.n_env = p->v.n_env;
    f.A = p->v.A;
    f.epb = p->v.geo_layout.epb;
    f.device_cus = p->device_cus;
    f.lane_polys = p->hgeo[1].present && !p->hgeo[1].env_off.empty() ? (long long)p->hgeo[1].env_off.back() : 0;
    f.has_geo = p->v.geo != nullptr;
    f.has_static = p->v.geo_layout.has[0];
    f.has_lanes = p->v.geo_layout.has[1];
    f.wgmap = p->v.wgmap != nullptr;
    f.overlapped = p->v.overlapped;
    f.fused_step = p->fused_step;
    f.grid_tier = p->grid_tier;
    f.side_models = side_models(p);
    f.scene_regen = p->scene_regen;
    f.ego_eligible = p->ego_kernel && p->v.A == 1 && p->all_boxes && !side_models(p) && !p->hgeo[1].present;
    f.iou = p->status_cfg.check_no_action || p->status_cfg.check_arrival;
    f.idm_on = p->idm.on;
    f.chain_steps = p->chain_steps;
    f.chain_loop = p->chain_loop;
    f.chain_pipe = p->chain_pipe;
    f.chain_pipe2 = p->chain_pipe2;
    f.split_steps = p->split_steps;
    f.chain_depth = p->chain_depth;
    f.shape64 = p->shape64;
    return f;
}

// what must hold before a stepping call enqueues anything for a pool with replayed participants
static int replay_check(t2d_pool* p, int interval_ms) {
    if (!p->replay_types) return T2D_OK;
    if (!p->replay_src)
        return fail(p, T2D_ERR_STATE, "the parameter table holds a T2D_MODEL_REPLAY row: t2d_replay_bind must precede the step");
    if (interval_ms % p->replay.period_ms != 0)
        return fail(p, T2D_ERR_INVALID, "interval_ms " + std::to_string(interval_ms) + " is not a multiple of the replay source's period (" +
                                            std::to_string(p->replay.period_ms) + " ms): there is no state between two stamps");
    return T2D_OK;
}

static int replay_impl(t2d_pool* p, int step_ms, hipStream_t s);   // (defined with t2d_replay_bind)

int t2d_integrate(t2d_pool* p, int32_t interval_ms, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_integrate");
    if (interval_ms <= 0) return fail(p, T2D_ERR_INVALID, "interval_ms must be positive");
    hipStream_t s = (hipStream_t)hip_stream;
    int rc;
    if ((rc = replay_check(p, interval_ms))) return rc;
    touch(p, s);
    if ((rc = prepare_interval(p, interval_ms, s))) return rc;
    if (p->idm.on && (rc = idm_impl(p, s))) return rc;
    if (p->has_drift && (rc = drift_impl(p, interval_ms, s))) return rc;
    if (p->replay_types && (rc = replay_impl(p, interval_ms, s))) return rc;
    if ((rc = record_event(p, 0, s, true))) return rc;
    // (four participants per lane pay where the model is cheap enough for the kernel to be memory-bound: measured at 4 M
    // participants 72.4 -> 63.5 us for point masses, 74.6 -> 73.7 for the kinematic bicycle, 167.7 -> 170.3 for the dynamics
    // model -- pools whose table holds a dynamics row keep one participant per lane)
    bool wide = true;
    for (int t = 0; t < p->v.n_types; ++t)   // (of the types some active participant HAS: t2d_reset keeps the set)
        wide = wide && !((p->types_used >> t & 1u) && (int)p->host_params[t][T2D_P_MODEL] == T2D_MODEL_DYNAMICS);
    int only_model = -1;   // the one model every active participant has, if there is one: an instantiation that carries it alone
    // (replayed participants become active whenever their recording says so, not at t2d_reset: their rows always count)
    const uint32_t used = p->types_used | p->replay_types;
    for (int t = 0; t < p->v.n_types; ++t)
        if (used >> t & 1u) {
            const int m = (int)p->host_params[t][T2D_P_MODEL];
            only_model = only_model == -1 || only_model == m ? m : -2;
        }
    T2D_HIP(p, t2d::launch_integrate(p->v, interval_ms, p->integrator_variant, wide, only_model, s));
    p->applied_spans_restart = false;   // (every active participant's T2D_F_APPLIED0 is this call's)
    return record_event(p, 0, s, false);
}

static void fill_idm(t2d::PoolView& v, t2d_pool* p) {
    v.idm_rows = p->idm.view.rows;
    v.idm_ctrl_all = p->idm.view.ctrl_id;
    v.idm_leader = p->idm.view.leader;
    v.idm_n_ctrl = p->idm.view.n_ctrl;
    v.idm_act0_own = (float*)p->field_ptr[T2D_F_ACT0];
    v.idm_act1_own = (float*)p->field_ptr[T2D_F_ACT1];
}

// Every launch with a status epilogue goes through here (collide_impl with_status, the multi-step launches of t2d_step_n): the
// epilogue may restart finished envs (auto-reset, regenerated scenes) and leaves T2D_F_APPLIED0 of the ended episode behind
static void status_step_enqueued(t2d_pool* p) { p->applied_spans_restart = p->auto_reset || p->scene_regen; }

// events (and status) of the poses as they are -- or, `step` = the plan of a fused one-launch step, the whole step
static int collide_impl(t2d_pool* p, bool with_status, int interval_ms, hipStream_t s, const StepPlan* step = nullptr) {
    int rc;
    touch(p, s);
    if (with_status) status_step_enqueued(p);
    const int fuse_variant = step ? p->integrator_variant : -1;
    const int kid = fuse_variant >= 0 ? 2 : 1;
    if ((rc = record_event(p, kid, s, true))) return rc;
    p->scene_committed_in_step = false;
    if (p->grid_tier) {   // the map's verdicts for the poses as they are now, ahead of the event kernel that ORs them in
        if (fuse_variant >= 0) return fail(p, T2D_ERR_STATE, "internal: a grid-tier pool took the fused step");
        T2D_HIP(p, t2d::launch_map_events(p->v, p->mapgrid, p->d_grid_seg, p->d_map_flags, s));
    }
    if (step && step->ego) {
        t2d::PoolView v = p->v;
        // staged scene regeneration: the step's own epilogue moves finished envs into their next lot (no launch behind it)
        if (with_status && p->scene_regen && p->scene.ring > 0 && p->d_scene_view) {
            v.regen = p->d_scene_view;
            p->scene_committed_in_step = p->scene_commit_used = true;
        }
        T2D_HIP(p, t2d::launch_ego_step(v, p->status_cfg, interval_ms, fuse_variant, s));
    } else {
        t2d::PoolView v = p->v;
        v.split_step = step && step->split;
        if (step && step->idm_fused) fill_idm(v, p);
        T2D_HIP(p, t2d::launch_collide(v, p->status_cfg, with_status, interval_ms, fuse_variant, s, step && step->w64));
    }
    return record_event(p, kid, s, false);
}

int t2d_collide(t2d_pool* p, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_collide");
    return collide_impl(p, false, 0, (hipStream_t)hip_stream);
}

// generated parking scenes with regeneration on: envs whose episode ended in the launch just enqueued move on to their next
// scene -- in that launch's own epilogue (ego step kernel) or in one cheap launch on the step's stream: staged scenes are
// copied in; every kSceneRefillPeriod steps the staging ring is topped up on the pool's own stream, off the critical path
// (one scene is a ~46 us single-lane chain).  The step stream waits for refill j before it launches refill j + 1, so the
// commits of steps [8 j, 8 j + 8) rely on refill j - 1 alone: it staged the 16 episodes past what it read at step >= 8 j - 8,
// and an env ends at most one episode in two steps -- 8 episodes by step 8 j + 8: half the ring is margin.  A slot a refill
// rewrites held an episode the env has left.  (Period 4 until round 4: the event wait + the side stream's three launches
// cost the step stream ~1 us per step on average, 36.2 -> 35.0 us per ParkingEnv vector step with period 8.)
constexpr int kSceneRing = 16;
constexpr int kSceneRefillPeriod = 8;
static int regenerate_done_scenes(t2d_pool* p, hipStream_t s) {
    if (!p->scene_regen) return T2D_OK;
    int rc;
    const bool refill = p->scene.ring > 0 && p->step_count % kSceneRefillPeriod == 0;
    if (refill && p->scene_refill_pending) T2D_HIP(p, hipStreamWaitEvent(s, p->ev_scene_refill, 0));
    if (!p->scene_committed_in_step) {   // (the ego step kernel has done it in its epilogue otherwise)
        if ((rc = record_event(p, 6, s, true))) return rc;
        if (p->scene.ring > 0) {   // staged scenes: sixteen lanes per env copy the prepared scene in
            T2D_HIP(p, t2d::launch_scene_commit(p->v, p->scene, p->v.n_env, s));
            p->scene_commit_used = true;
        } else {
            T2D_HIP(p, t2d::launch_parking_scenes(p->v, p->scene, p->v.n_env, 2, s));
        }
        if ((rc = record_event(p, 6, s, false))) return rc;
    }
    if (refill) {
        T2D_HIP(p, hipEventRecord(p->ev_scene_commit, s));
        T2D_HIP(p, hipStreamWaitEvent(p->scene_stream, p->ev_scene_commit, 0));
        T2D_HIP(p, t2d::launch_scene_refill(p->scene, p->v.n_env, p->scene_stream));
        T2D_HIP(p, hipEventRecord(p->ev_scene_refill, p->scene_stream));
        p->scene_refill_pending = true;
    }
    return T2D_OK;
}

// this step's slot of the record ring; a gather still reading that slot (enqueued RING steps ago or less) is waited for
// on the step's stream first -- an event wait, nothing blocks the host
static int claim_record_slot(t2d_pool* p, hipStream_t s) {
    const int k = (int)(p->step_count % T2D_RECORD_RING);
    if (hipEvent_t e = p->slot_event[k]) {   // one wait covers every slot that gather reads (one event per gather)
        T2D_HIP(p, hipStreamWaitEvent(s, e, 0));
        for (hipEvent_t& q : p->slot_event)
            if (q == e) q = nullptr;
    }
    p->v.record = (uint2*)p->field_ptr[T2D_F_RECORD] + (size_t)k * p->v.n_env;
    return T2D_OK;
}

int t2d_check_status(t2d_pool* p, int32_t interval_ms, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_check_status");
    if (interval_ms <= 0) return fail(p, T2D_ERR_INVALID, "interval_ms must be positive");
    int rc;
    if ((rc = claim_record_slot(p, (hipStream_t)hip_stream))) return rc;
    rc = collide_impl(p, true, interval_ms, (hipStream_t)hip_stream);
    if (rc == T2D_OK) p->step_count++;
    if (rc == T2D_OK) rc = regenerate_done_scenes(p, (hipStream_t)hip_stream);
    return rc;
}

int t2d_step(t2d_pool* p, int32_t interval_ms, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    const StepPlan plan = plan_step(step_facts(p), 1);
    if (!plan.fused) {
        int rc = t2d_integrate(p, interval_ms, hip_stream);
        if (rc != T2D_OK) return rc;
        return t2d_check_status(p, interval_ms, hip_stream);
    }
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_step");
    if (interval_ms <= 0) return fail(p, T2D_ERR_INVALID, "interval_ms must be positive");
    int rc;
    if ((rc = replay_check(p, interval_ms))) return rc;
    if ((rc = prepare_interval(p, interval_ms, (hipStream_t)hip_stream))) return rc;
    if ((rc = claim_record_slot(p, (hipStream_t)hip_stream))) return rc;
    // (installed IDM controllers: a launch of their own ahead of the step -- or, plan.idm_fused, the front of the step launch)
    if (p->idm.on && !plan.idm_fused && (rc = idm_impl(p, (hipStream_t)hip_stream))) return rc;
    if (p->has_drift && (rc = drift_impl(p, interval_ms, (hipStream_t)hip_stream))) return rc;
    if (p->replay_types && (rc = replay_impl(p, interval_ms, (hipStream_t)hip_stream))) return rc;
    rc = collide_impl(p, true, interval_ms, (hipStream_t)hip_stream, &plan);
    if (rc == T2D_OK) p->step_count++;
    if (rc == T2D_OK) rc = regenerate_done_scenes(p, (hipStream_t)hip_stream);
    return rc;
}

int t2d_step_n(t2d_pool* p, int32_t interval_ms, int32_t n_steps, int64_t act_step_stride, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (n_steps < 1 || act_step_stride < 0) return fail(p, T2D_ERR_INVALID, "n_steps must be >= 1 and act_step_stride >= 0");
    // (the pool's own action fields hold ONE action set: a ring needs bound memory of n_steps * act_step_stride elements)
    if (act_step_stride != 0 && p->v.act0 == (const float*)p->field_ptr[T2D_F_ACT0])
        return fail(p, T2D_ERR_INVALID, "act_step_stride > 0 needs an action ring bound with t2d_bind_actions (the pool's own ACT0 / ACT1 hold one set)");
    // a declared extent (t2d_set_action_extent) is held against the furthest element step n_steps - 1 reads
    if (p->act_extent && (int64_t)(p->v.N - 1) * p->v.act_stride + (int64_t)(n_steps - 1) * act_step_stride >= p->act_extent)
        return fail(p, T2D_ERR_INVALID, "step " + std::to_string(n_steps - 1) + " of the fragment would read past the declared extent of the bound actions (" +
                                         std::to_string((long long)p->act_extent) + " elements)");
    if (p->chain_failed || p->scene_commit_failed) return report_chain_failure(p);   // (once; the call after it goes ahead with plain launches)
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_step_n");
    if (interval_ms <= 0) return fail(p, T2D_ERR_INVALID, "interval_ms must be positive");
    hipStream_t s = (hipStream_t)hip_stream;
    const StepPlan plan = plan_step(step_facts(p), n_steps);
    const float *a0 = p->v.act0, *a1 = p->v.act1;
    int rc = T2D_OK;
    if (!plan.multi) {   // step by step
        for (int k = 0; k < n_steps && rc == T2D_OK; ++k) {
            p->v.act0 = a0 + (size_t)k * act_step_stride;
            p->v.act1 = a1 + (size_t)k * act_step_stride;
            rc = t2d_step(p, interval_ms, hip_stream);
        }
        p->v.act0 = a0;
        p->v.act1 = a1;
        return rc;
    }
    touch(p, s);
    if ((rc = prepare_interval(p, interval_ms, s))) return rc;
    status_step_enqueued(p);
    for (int done = 0; done < n_steps && rc == T2D_OK;) {
        // one launch covers at most a ring of record slots (and a gather that still reads any of them is waited for first)
        int n = std::min(n_steps - done, (int)T2D_RECORD_RING);
        // the chained form of large pools: chain_depth steps per workgroup (launches of a multiple of it; what is left over
        // at the end of a call goes out one step per workgroup)
        const int depth = plan.chain_k > 1 && n >= plan.chain_k ? plan.chain_k : 1;
        n -= n % depth;
        const int slot0 = (int)(p->step_count % T2D_RECORD_RING);
        for (int k = 0; k < n; ++k) {
            if ((rc = claim_record_slot(p, s))) return rc;
            p->step_count++;
        }
        t2d::PoolView v = p->v;
        v.wgmap = nullptr;
        v.overlapped = p->chain_priority;
        v.act0 = a0 + (size_t)done * act_step_stride;
        v.act1 = a1 + (size_t)done * act_step_stride;
        v.chain_done = p->d_chain;
        v.chain_err = reinterpret_cast<uint32_t*>(p->d_chain + p->chain_slots);
        v.chain_base = p->chain_count;
        v.chain_act_step = act_step_stride;
        v.split_step = plan.split;
        v.pipe_step = plan.pipe;
        v.chain_real_wgs = plan.real_wgs;
        if (plan.idm_fused) fill_idm(v, p);
        v.record_ring = (uint2*)p->field_ptr[T2D_F_RECORD];
        v.record_slot0 = slot0;
        // CHAIN forms (one workgroup per (env set, step), ordered by the counters in d_chain): the counters continue from
        // launch to launch only while the launches have one shape -- a pool that changes form (t2d_set_idm, new geometry,
        // t2d_set_split_step, t2d_set_step_chaining) starts them afresh, on the stream -- and every fragment carries the
        // checkpoint a failed hand-off is rolled back to
        const bool chain_form = !plan.ego && !plan.loop;
        v.chain_k = chain_form && !plan.split && depth > 1 ? depth : 0;
        v.loop_steps = v.chain_k ? v.chain_k : plan.loop ? n : 0;
        if (chain_form) {
            const uint32_t sig = ((uint32_t)v.chain_real_wgs << 1) | (v.split_step ? 1u : 0u) | 0x80000000u;
            if (sig != p->chain_sig) {
                T2D_HIP(p, hipMemsetAsync(p->d_chain, 0, sizeof(unsigned long long) * (size_t)p->chain_slots, s));
                p->chain_count = 0;
                p->chain_sig = sig;
                v.chain_base = 0;
            }
            if (!p->d_ckpt) {
                const size_t words = 7 * (size_t)p->v.N + 2 * (size_t)p->v.n_env;
                T2D_HIP(p, p->d_ckpt.alloc_zeroed(words));
            }
            v.ckpt = p->d_ckpt;
            v.ckpt_tag = (uint32_t)(p->step_count - n);   // (low half of the step count this fragment starts from)
            v.chain_fault = p->chain_fault;
        } else {
            v.ckpt = nullptr;
            v.chain_fault = 0;
        }
        // (the checkpoint is what a failure is rolled back to only while every multi-step launch since the last host
        // synchronisation carried one)
        p->ckpt_armed = chain_form && (p->chain_used ? p->ckpt_armed : true);
        if ((rc = record_event(p, 7, s, true))) return rc;
        if (plan.ego) T2D_HIP(p, t2d::launch_ego_step(v, p->status_cfg, interval_ms, p->integrator_variant, s));
        else T2D_HIP(p, t2d::launch_step_chain(v, p->status_cfg, interval_ms, p->integrator_variant, n, s, plan.w64));
        if ((rc = record_event(p, 7, s, false))) return rc;
        if (chain_form) p->chain_count += (uint32_t)n;   // (only these launches move the counters)
        p->chain_used = true;
        done += n;
    }
    p->v.record = (uint2*)p->field_ptr[T2D_F_RECORD] + (size_t)((p->step_count + T2D_RECORD_RING - 1) % T2D_RECORD_RING) * p->v.n_env;
    return rc;
}

int t2d_step_form(t2d_pool* p, int32_t n_steps) {
    if (!p) return -1;
    return plan_step(step_facts(p), n_steps).form;   // (the plan t2d_step / t2d_step_n launch from)
}

int t2d_set_split_step(t2d_pool* p, int32_t on) {
    if (!p) return T2D_ERR_INVALID;
    p->split_steps = on != 0;
    return T2D_OK;
}

int t2d_set_step_chaining(t2d_pool* p, int32_t on, int32_t priority_rule) {
    if (!p) return T2D_ERR_INVALID;
    p->chain_steps = on != 0;
    p->chain_loop = on != 2;   // 2: always the chained form, also for small pools (measurements)
    p->chain_pipe = on == 1 || on == 4;   // 3: small pools loop without the integrator waves (measurements, tests)
    p->chain_pipe2 = on == 1;             // 4: integrator waves, but no lane waves
    p->chain_priority = priority_rule != 0;
    return T2D_OK;
}

int t2d_step_groups(t2d_pool* const* pools, const float* const* act0_dev, const float* const* act1_dev,
                    void* const* hip_streams, int32_t n, int32_t interval_ms) {
    if (!pools || !hip_streams || n <= 0 || (act0_dev == nullptr) != (act1_dev == nullptr)) return T2D_ERR_INVALID;
    for (int i = 0; i < n; ++i) {
        int rc;
        if (!pools[i]) return T2D_ERR_INVALID;
        if (act0_dev && (rc = t2d_bind_actions(pools[i], act0_dev[i], act1_dev[i])) != T2D_OK) return rc;
        pools[i]->v.overlapped = n > 1;   // several groups in flight: the kernels' wave priorities favour retiring workgroups
        rc = t2d_step(pools[i], interval_ms, hip_streams[i]);
        pools[i]->v.overlapped = 0;
        if (rc != T2D_OK) return rc;
    }
    return T2D_OK;
}

int t2d_set_fused_step(t2d_pool* p, int32_t on) {
    if (!p) return T2D_ERR_INVALID;
    p->fused_step = on != 0;
    return T2D_OK;
}

int t2d_set_ego_kernel(t2d_pool* p, int32_t on) {
    if (!p) return T2D_ERR_INVALID;
    p->ego_kernel = on != 0;
    return T2D_OK;
}

int t2d_snapshot(t2d_pool* p) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->have_reset) return fail(p, T2D_ERR_STATE, "t2d_reset must precede t2d_snapshot");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    const size_t nb = 4 * (size_t)p->v.N;
    float* src[6] = {p->v.x, p->v.y, p->v.heading, p->v.speed, p->v.vx, p->v.vy};
    for (int k = 0; k < 6; ++k) {
        if (!p->d_snap[k]) T2D_HIP(p, p->d_snap[k].alloc((size_t)p->v.N));
        T2D_HIP(p, hipMemcpy(p->d_snap[k], src[k], nb, hipMemcpyDeviceToDevice));
    }
    for (int k = 0; k < 2; ++k) {
        if (!p->d_snap_omega[k]) T2D_HIP(p, p->d_snap_omega[k].alloc((size_t)p->v.N));
        T2D_HIP(p, hipMemcpy(p->d_snap_omega[k], k ? p->v.omega_r : p->v.omega_f, nb, hipMemcpyDeviceToDevice));
        p->v.snap_omega[k] = p->has_drift ? p->d_snap_omega[k] : nullptr;
    }
    if (!p->d_snap_ids) T2D_HIP(p, p->d_snap_ids.alloc((size_t)p->v.N));
    T2D_HIP(p, hipMemcpy(p->d_snap_ids, p->v.ids, nb, hipMemcpyDeviceToDevice));
    T2D_HIP(p, hipMemcpy(p->d_snap_min_dist, p->d_min_dist, sizeof(double) * p->v.n_env, hipMemcpyDeviceToDevice));
    p->have_snapshot = true;
    p->snap_types = p->types_used;   // (the ids just copied: t2d_restore and the auto-reset write them back)
    for (int k = 0; k < 6; ++k) p->v.snap[k] = p->d_snap[k];
    p->v.snap_ids = p->d_snap_ids;
    p->v.auto_reset = p->auto_reset ? 1 : 0;
    return T2D_OK;
}

int t2d_set_auto_reset(t2d_pool* p, int32_t on) {
    if (!p) return T2D_ERR_INVALID;
    if (on && !p->have_snapshot) return fail(p, T2D_ERR_STATE, "t2d_snapshot must precede t2d_set_auto_reset");
    p->auto_reset = on != 0;
    p->v.auto_reset = p->auto_reset ? 1 : 0;
    if (p->auto_reset) p->types_used |= p->snap_types;   // (the integrator's instantiation must carry the snapshot's models)
    return T2D_OK;
}

int t2d_restore(t2d_pool* p, int32_t mode, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->have_snapshot) return fail(p, T2D_ERR_STATE, "t2d_snapshot must precede t2d_restore");
    if (mode != 0 && mode != 1) return fail(p, T2D_ERR_INVALID, "mode must be 0 (all) or 1 (done envs)");
    touch(p, (hipStream_t)hip_stream);
    if (mode == 0) p->chain_failed = false;   // (see t2d_reset)
    T2D_HIP(p, t2d::launch_restore(p->v, p->v.snap, p->v.snap_ids, mode, (hipStream_t)hip_stream));
    p->types_used |= p->snap_types;
    return T2D_OK;
}

int t2d_parking_scenes(t2d_pool* p, uint64_t seed, int64_t first_env, int64_t env_stride, double type_proportion,
                       double vehicle_length, double vehicle_width, int32_t regenerate) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->have_params) return fail(p, T2D_ERR_STATE, "t2d_set_param_table must precede t2d_parking_scenes");
    if (p->v.A != 1) return fail(p, T2D_ERR_INVALID, "generated parking scenes need a pool with one participant per env");
    if (p->has_drift) return fail(p, T2D_ERR_INVALID, "SingleTrackDrift agents are not supported in generated parking scenes");
    if (p->replay_types) return fail(p, T2D_ERR_INVALID, "replayed participants are not supported in generated parking scenes");
    if (p->hgeo[1].present) return fail(p, T2D_ERR_STATE, "lane geometry cannot be combined with generated parking scenes");
    if (env_stride < 0) return fail(p, T2D_ERR_INVALID, "env_stride must be >= 0");
    if (regenerate != 0 && regenerate != 1 && regenerate != 2)
        return fail(p, T2D_ERR_INVALID, "regenerate must be 0 (off), 1 (staged ahead) or 2 (generated in the step's stream)");
    if (vehicle_length < vehicle_width || !(vehicle_length > 0.0) || !(vehicle_width > 0.0)) {
        vehicle_length = 5.3;  // ParkingLotGenerator.__init__ :45-57
        vehicle_width = 2.5;
    }
    if (!(type_proportion >= 0.0)) type_proportion = 0.0;
    if (type_proportion > 1.0) type_proportion = 1.0;
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    ++p->geo_gen;
    const int E = p->v.n_env;
    constexpr int K = T2D_GEN_MAX_QUADS;
    int rc;
    // geometry records in capacity layout: K polygon slots of 4 vertices per env, a dead slot = a box nothing meets
    t2d::GeoLayout gl{};
    const int log2A = log2_pad(1);
    int epb = 256 >> log2A;
    for (;; epb >>= 1) {
        const int mp[2] = {K * epb, 0}, mv[2] = {4 * K * epb, 0};
        fill_layout(gl, epb, mp, mv);
        if (gl.stride <= 8192) break;
        if ((epb << log2A) <= 64) return fail(p, T2D_ERR_GEOMETRY, "scene record exceeds the 32 KiB LDS record");
    }
    gl.has[0] = 1;
    gl.has[1] = 0;
    const int nb = (E + epb - 1) / epb;
    {
        std::vector<uint32_t> rec((size_t)nb * gl.stride, 0u);
        const float dead[4] = {INFINITY, -INFINITY, INFINITY, -INFINITY};
        for (int b = 0; b < nb; ++b) {
            uint32_t* r = rec.data() + (size_t)b * gl.stride;
            int32_t* pstart = reinterpret_cast<int32_t*>(r) + gl.off_pstart[0];
            int32_t* vstart = reinterpret_cast<int32_t*>(r) + gl.off_vstart[0];
            for (int el = 0; el <= epb; ++el) pstart[el] = K * el;
            for (int q = 0; q <= K * epb; ++q) vstart[q] = 4 * q;
            float* bb = reinterpret_cast<float*>(r) + gl.off_aabb[0];
            for (int q = 0; q < K * epb; ++q) memcpy(bb + 4 * q, dead, sizeof dead);
        }
        if ((rc = dev_replace(p, &p->d_geo, rec.data(), rec.size()))) return rc;
    }
    p->hgeo[0] = t2d_pool::HostGeo{};
    p->v.geo = p->d_geo;
    p->v.geo_layout = gl;
    p->v.wgmap = nullptr;   // the launch shape may have changed
    {
        std::vector<float> zf(4 * (size_t)E, 0.f);
        std::vector<double> zd(8 * (size_t)E, 0.0);
        if ((rc = dev_replace(p, &p->d_boundary, zf.data(), zf.size()))) return rc;
        if ((rc = dev_replace<uint8_t>(p, &p->d_boundary_valid, nullptr, 0))) return rc;
        if ((rc = dev_replace(p, &p->d_target_xy, zd.data(), 8 * (size_t)E))) return rc;
        if ((rc = dev_replace(p, &p->d_target_c, zd.data(), 2 * (size_t)E))) return rc;
        std::vector<float> zl(16 * (size_t)K * E, 0.f);   // 4 edge records of 4 floats per polygon slot
        std::vector<int32_t> zi(E, 0);
        if ((rc = dev_replace(p, &p->d_lidar_xy, zl.data(), zl.size()))) return rc;
        if ((rc = dev_replace(p, &p->d_lidar_cnt, zi.data(), zi.size()))) return rc;
        std::vector<uint8_t> zm(4 * (size_t)K * E, 0xff);   // per edge: its ring's slot if the ring may cull (install_quad_slot)
        if ((rc = dev_replace(p, &p->d_lidar_meta, zm.data(), zm.size()))) return rc;
    }
    p->v.boundary = p->d_boundary;
    p->v.boundary_valid = nullptr;
    p->v.target_xy = p->d_target_xy;
    p->v.target_c = p->d_target_c;
    p->have_target = true;
    const size_t nbytes = 4 * (size_t)p->v.N;
    for (int k = 0; k < 6; ++k)
        if (!p->d_snap[k]) T2D_HIP(p, p->d_snap[k].alloc((size_t)p->v.N));
    if (!p->d_snap_ids) T2D_HIP(p, p->d_snap_ids.alloc((size_t)p->v.N));
    // the per-scene arrays (layout of t2d_generate_parking's outputs): live [E] + the staging ring [E * ring] used when
    // scenes are regenerated (regenerate == 1; == 2 generates on the step's stream instead), episode counters
    const int ring = regenerate == 1 ? kSceneRing : 0;
    const size_t per[8] = {(size_t)K * 8 * sizeof(float), (size_t)K * sizeof(int32_t), sizeof(int32_t), 3 * sizeof(double),
                           8 * sizeof(float), sizeof(double), 4 * sizeof(float), sizeof(uint32_t)};
    const size_t counts[2] = {(size_t)E, (size_t)E * ring};
    size_t off[21], total = 0;
    for (int set = 0; set < 2; ++set)
        for (int k = 0; k < 8; ++k) {
            off[8 * set + k] = total;
            total += (per[k] * counts[set] + 255) & ~(size_t)255;
        }
    off[16] = total; total += ((size_t)E * sizeof(int32_t) + 255) & ~(size_t)255;          // episode
    off[17] = total; total += ((size_t)E * ring * sizeof(int32_t) + 255) & ~(size_t)255;   // staged_ep
    off[18] = total; total += 256;                                                         // commit_err
    off[19] = total; total += 256;                                                         // refill_count
    off[20] = total; total += ((size_t)E * ring * sizeof(uint2) + 255) & ~(size_t)255;     // refill_list
    if (p->scene_stream) T2D_HIP(p, hipStreamSynchronize(p->scene_stream));
    T2D_HIP(p, p->d_scene_arrays.alloc_zeroed(total));   // (frees the previous arrays first)
    char* base = (char*)p->d_scene_arrays.get();
    t2d::SceneView& sv = p->scene;
    sv = t2d::SceneView{};
    sv.seed = seed; sv.first_env = first_env; sv.env_stride = env_stride;
    sv.type_proportion = type_proportion; sv.len = vehicle_length; sv.wid = vehicle_width;
    t2d::SceneArrays* sets[2] = {&sv.live, &sv.staged};
    for (int set = 0; set < 2; ++set) {
        char* b = base;
        *sets[set] = t2d::SceneArrays{(float*)(b + off[8 * set + 0]), (int32_t*)(b + off[8 * set + 1]), (int32_t*)(b + off[8 * set + 2]),
                                      (double*)(b + off[8 * set + 3]), (float*)(b + off[8 * set + 4]), (double*)(b + off[8 * set + 5]),
                                      (float*)(b + off[8 * set + 6]), (uint32_t*)(b + off[8 * set + 7])};
    }
    sv.episode = (int32_t*)(base + off[16]);
    sv.staged_ep = (int32_t*)(base + off[17]);
    sv.commit_err = (uint32_t*)(base + off[18]);
    sv.refill_count = (uint32_t*)(base + off[19]);
    sv.refill_list = (uint2*)(base + off[20]);
    p->scene_commit_used = p->scene_commit_failed = false;
    sv.ring = ring;
    if (ring > 0) {
        T2D_HIP(p, hipMemset(sv.staged_ep, 0xff, (size_t)E * ring * sizeof(int32_t)));   // -1 = empty slot
        if (!p->scene_stream) T2D_HIP(p, hipStreamCreateWithFlags(&p->scene_stream, hipStreamNonBlocking));
        if (!p->ev_scene_commit) T2D_HIP(p, hipEventCreateWithFlags(&p->ev_scene_commit, hipEventDisableTiming));
        if (!p->ev_scene_refill) T2D_HIP(p, hipEventCreateWithFlags(&p->ev_scene_refill, hipEventDisableTiming));
    }
    p->scene_refill_pending = false;
    sv.geo = p->d_geo; sv.gl = gl;
    sv.lidar_xy = p->d_lidar_xy; sv.lidar_cnt = p->d_lidar_cnt; sv.lidar_meta = p->d_lidar_meta;
    sv.boundary = p->d_boundary; sv.target_xy = p->d_target_xy; sv.target_c = p->d_target_c;
    for (int k = 0; k < 6; ++k) sv.snap[k] = p->d_snap[k];
    sv.snap_ids = p->d_snap_ids;
    sv.snap_min_dist = p->d_snap_min_dist;
    sv.ids_word = ((uint32_t)(int)p->host_params[0][T2D_P_MODEL] << t2d::kIdsModelShift) | (0u << t2d::kIdsTypeShift) |
                  (1u << t2d::kIdsActiveShift);
    p->scene_mode = true;
    p->scene_regen = regenerate != 0;
    if (!p->d_scene_view) T2D_HIP(p, p->d_scene_view.alloc(1));
    T2D_HIP(p, hipMemcpy(p->d_scene_view, &sv, sizeof(sv), hipMemcpyHostToDevice));   // (what the ego step kernel's epilogue reads)
    if ((rc = rebuild_lidar_geo(p))) return rc;
    {  // t2d_reset's remaining columns: wheel speeds start at zero
        for (int f : {T2D_F_OMEGA_F, T2D_F_OMEGA_R}) T2D_HIP(p, hipMemset(p->field_ptr[f], 0, nbytes));
    }
    touch(p, nullptr);   // the two set-up launches below run on the null stream
    T2D_HIP(p, t2d::launch_parking_scenes(p->v, sv, E, 1, nullptr));
    if (ring > 0) T2D_HIP(p, t2d::launch_scene_refill(sv, E, nullptr));   // episodes 1 .. ring of every env
    T2D_HIP(p, quiesce(p));
    p->have_reset = true;
    p->have_snapshot = true;
    p->snap_types |= 1u;   // (every scene's agent is type 0: sv.ids_word, in the pool and in the snapshot)
    p->types_used |= 1u;
    for (int k = 0; k < 6; ++k) p->v.snap[k] = p->d_snap[k];
    p->v.snap_ids = p->d_snap_ids;
    p->v.snap_omega[0] = p->v.snap_omega[1] = nullptr;
    p->v.auto_reset = p->auto_reset ? 1 : 0;
    if (p->rs_follow_on) return t2d_rs_follow_reset(p, nullptr, nullptr);
    return T2D_OK;
}

int t2d_get_parking_scenes(t2d_pool* p, float* quads, int32_t* quad_id, int32_t* n_quads, double* start, float* target,
                           double* target_heading, float* boundary, uint32_t* info, int32_t* episode) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->scene_mode) return fail(p, T2D_ERR_STATE, "t2d_parking_scenes has not been called on this pool");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    const size_t E = (size_t)p->v.n_env;
    constexpr size_t K = T2D_GEN_MAX_QUADS;
    const t2d::SceneView& sv = p->scene;
    if (quads) T2D_HIP(p, hipMemcpy(quads, sv.live.quads, E * K * 8 * sizeof(float), hipMemcpyDeviceToHost));
    if (quad_id) T2D_HIP(p, hipMemcpy(quad_id, sv.live.quad_id, E * K * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (n_quads) T2D_HIP(p, hipMemcpy(n_quads, sv.live.n_quads, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (start) T2D_HIP(p, hipMemcpy(start, sv.live.start, E * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (target) T2D_HIP(p, hipMemcpy(target, sv.live.target, E * 8 * sizeof(float), hipMemcpyDeviceToHost));
    if (target_heading) T2D_HIP(p, hipMemcpy(target_heading, sv.live.target_heading, E * sizeof(double), hipMemcpyDeviceToHost));
    if (boundary) T2D_HIP(p, hipMemcpy(boundary, sv.live.boundary, E * 4 * sizeof(float), hipMemcpyDeviceToHost));
    if (info) T2D_HIP(p, hipMemcpy(info, sv.live.info, E * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (episode) T2D_HIP(p, hipMemcpy(episode, sv.episode, E * sizeof(int32_t), hipMemcpyDeviceToHost));
    return T2D_OK;
}

#ifdef T2D_DEBUG_HOOKS   // include/t2d_debug.h: libt2d_hip_debug.so only
int t2d_debug_memory(int64_t out[4]) {
    if (!out) return T2D_ERR_INVALID;
    for (int k = 0; k < 4; ++k) out[k] = t2d::g_mem_live[k].load(std::memory_order_relaxed);
    return T2D_OK;
}
#endif

#ifdef T2D_TIMING
// profiling builds only (not part of the ABI): read and clear the phase cycle accumulators
int t2d_debug_read(t2d_pool* p, unsigned long long* out, size_t n_words) {
    if (!p || !p->v.dbg) return T2D_ERR_INVALID;
    T2D_HIP(p, quiesce(p));
    T2D_HIP(p, hipMemcpy(out, p->v.dbg, n_words * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return T2D_OK;
}
#endif

// ---- multi-GPU: the all-gather of the per-env result records ------------------------------------------
int t2d_comm_unique_id(uint8_t* id) {
    if (!id) return T2D_ERR_INVALID;
    if (!rccl().ok) return fail(nullptr, T2D_ERR_HIP, rccl().err);
    ncclUniqueId u;
    const ncclResult_t r = rccl().GetUniqueId(&u);
    if (r != ncclSuccess) return fail(nullptr, T2D_ERR_HIP, std::string("ncclGetUniqueId: ") + rccl().GetErrorString(r));
    static_assert(sizeof(u) == T2D_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
    memcpy(id, &u, sizeof(u));
    return T2D_OK;
}

static int ensure_gather_objects(t2d_pool* p) {
    if (p->gather_stream) return T2D_OK;
    // Lowest stream priority: the collective's workgroups take the slots the step kernel leaves free at
    // its start and tail instead of displacing step workgroups out of the one-wave-round launch.
    int prio_least = 0, prio_greatest = 0;
    T2D_HIP(p, hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest));
    T2D_HIP(p, hipStreamCreateWithPriority(&p->gather_stream, hipStreamNonBlocking, prio_least));
    T2D_HIP(p, hipEventCreateWithFlags(&p->ev_frag_ready, hipEventDisableTiming));
    for (hipEvent_t& e : p->ev_gather) T2D_HIP(p, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    return T2D_OK;
}

int t2d_comm_init(t2d_pool* p, const uint8_t* id, int32_t rank, int32_t world) {
    if (!p) return T2D_ERR_INVALID;
    if (world < 1 || rank < 0 || rank >= world) return fail(p, T2D_ERR_INVALID, "t2d_comm_init: need 0 <= rank < world");
    if (world > 1 && !id) return fail(p, T2D_ERR_INVALID, "t2d_comm_init: the communicator id of t2d_comm_unique_id is required");
    T2D_HIP(p, hipSetDevice(p->device));
    int rc;
    if ((rc = ensure_gather_objects(p))) return rc;
    if (p->comm) {
        (void)rccl().CommDestroy((ncclComm_t)p->comm);
        p->comm = nullptr;
    }
    p->comm_rank = rank;
    p->comm_world = world;
    if (!id) return T2D_OK;   // a world of one without RCCL: t2d_gather degenerates to a copy on the gather stream
    if (!rccl().ok) return fail(p, T2D_ERR_HIP, rccl().err);
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t c = nullptr;
    const ncclResult_t r = rccl().CommInitRank(&c, world, u, rank);
    if (r != ncclSuccess) return fail(p, T2D_ERR_HIP, std::string("ncclCommInitRank: ") + rccl().GetErrorString(r));
    p->comm = c;
    return T2D_OK;
}

#ifdef T2D_DEBUG_HOOKS   // include/t2d_debug.h: libt2d_hip_debug.so only
int t2d_debug_delay_gather(t2d_pool* p, int32_t microseconds) {
    if (!p) return T2D_ERR_INVALID;
    if (microseconds < 0 || microseconds > 200000) return fail(p, T2D_ERR_INVALID, "delay must be 0 .. 200000 us");
    T2D_HIP(p, hipSetDevice(p->device));
    int rc;
    if ((rc = ensure_gather_objects(p))) return rc;
    T2D_HIP(p, t2d::launch_spin(100ll * microseconds, p->gather_stream));
    return T2D_OK;
}
#endif

int t2d_comm_info(t2d_pool* p, int32_t* native_rccl, int32_t* world, int32_t* rank) {
    if (!p) return T2D_ERR_INVALID;
    int w = p->comm_world, r = p->comm_rank;
    if (p->comm) {   // what the communicator itself says, not what the caller passed to t2d_comm_init
        if (!rccl().CommCount || !rccl().CommUserRank) return fail(p, T2D_ERR_HIP, "librccl lacks ncclCommCount / ncclCommUserRank");
        ncclResult_t e = rccl().CommCount((ncclComm_t)p->comm, &w);
        if (e == ncclSuccess) e = rccl().CommUserRank((ncclComm_t)p->comm, &r);
        if (e != ncclSuccess) return fail(p, T2D_ERR_HIP, std::string("ncclCommCount: ") + rccl().GetErrorString(e));
    }
    if (native_rccl) *native_rccl = p->comm != nullptr;
    if (world) *world = w;
    if (rank) *rank = r;
    return T2D_OK;
}

int64_t t2d_step_count(const t2d_pool* p) { return p ? (int64_t)p->step_count : -1; }

int t2d_gather(t2d_pool* p, void* nccl_comm, int32_t n_steps, void* out_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!out_dev) return fail(p, T2D_ERR_INVALID, "t2d_gather: out_dev is null");
    if (n_steps < 1 || T2D_RECORD_RING % n_steps || p->step_count < n_steps || p->step_count % n_steps)
        return fail(p, T2D_ERR_INVALID, "t2d_gather: n_steps must divide the record ring (" + std::to_string(T2D_RECORD_RING) +
                                            ") and the step count (" + std::to_string(p->step_count) + ") must be a positive multiple of it");
    T2D_HIP(p, hipSetDevice(p->device));
    int rc;
    if ((rc = ensure_gather_objects(p))) return rc;
    ncclComm_t comm = nccl_comm ? (ncclComm_t)nccl_comm : (ncclComm_t)p->comm;
    if (!comm && p->comm_world > 1) return fail(p, T2D_ERR_STATE, "t2d_gather: no communicator (t2d_comm_init)");
    if (comm && !rccl().ok) return fail(p, T2D_ERR_HIP, rccl().err);
    hipStream_t s = (hipStream_t)hip_stream;
    const int first = (int)((p->step_count - n_steps) % T2D_RECORD_RING);   // contiguous: n_steps divides the ring
    const size_t count = (size_t)n_steps * p->v.n_env * 2;                  // u32 words of this rank's fragment
    const uint32_t* src = (const uint32_t*)p->field_ptr[T2D_F_RECORD] + (size_t)first * p->v.n_env * 2;
    // the gather stream picks up after the fragment's last step; the step stream does not wait for the collective
    T2D_HIP(p, hipEventRecord(p->ev_frag_ready, s));
    T2D_HIP(p, hipStreamWaitEvent(p->gather_stream, p->ev_frag_ready, 0));
    if (comm) {
        const ncclResult_t r = rccl().AllGather(src, out_dev, count, ncclUint32, comm, p->gather_stream);
        if (r != ncclSuccess) return fail(p, T2D_ERR_HIP, std::string("ncclAllGather: ") + rccl().GetErrorString(r));
    } else {
        T2D_HIP(p, hipMemcpyAsync(out_dev, src, count * sizeof(uint32_t), hipMemcpyDeviceToDevice, p->gather_stream));
    }
    hipEvent_t done = p->ev_gather[first];
    T2D_HIP(p, hipEventRecord(done, p->gather_stream));
    for (int k = first; k < first + n_steps; ++k) p->slot_event[k] = done;   // whoever overwrites these slots waits for it
    p->last_gather = done;
    return T2D_OK;
}

int t2d_gather_wait(t2d_pool* p, void* hip_stream, int32_t block_host) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->last_gather) return T2D_OK;
    T2D_HIP(p, hipSetDevice(p->device));
    if (block_host) T2D_HIP(p, hipEventSynchronize(p->last_gather));
    else T2D_HIP(p, hipStreamWaitEvent((hipStream_t)hip_stream, p->last_gather, 0));
    return T2D_OK;
}

// test hook: the next CHAIN launches of the pool break one hand-off on purpose (include/t2d.h)
#ifdef T2D_DEBUG_HOOKS   // include/t2d_debug.h: libt2d_hip_debug.so only
const char* t2d_debug_last_step_kernel(void) { return t2d::last_collide_form(); }
int t2d_debug_last_step_shape(void) { return t2d::last_collide_shape(); }
int t2d_debug_set_step_shape64(t2d_pool* p, int32_t on) {
    if (!p) return T2D_ERR_INVALID;
    p->shape64 = on != 0;
    return T2D_OK;
}

// the step kernel's slot hand-out, one wave per vector of 64 counts (include/t2d_debug.h)
int t2d_debug_wave_scan(int32_t device_id, int32_t n_waves, const int32_t* cnt_host, int32_t* off_host, int32_t* total_host) {
    if (n_waves < 1 || n_waves > T2D_WAVE_SCAN_MAX_WAVES)
        return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_wave_scan: n_waves must be in [1, T2D_WAVE_SCAN_MAX_WAVES]");
    if (!cnt_host || !off_host || !total_host) return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_wave_scan: a null array");
    int n_dev = 0;
    T2D_HIP(nullptr, hipGetDeviceCount(&n_dev));
    if (device_id < 0 || device_id >= n_dev) return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_wave_scan: no such device");
    T2D_HIP(nullptr, hipSetDevice(device_id));
    t2d::DevBuf<int32_t> cnt, out;   // (freed on every way out)
    T2D_HIP(nullptr, cnt.alloc((size_t)n_waves * 64));
    T2D_HIP(nullptr, out.alloc((size_t)n_waves * 65));
    T2D_HIP(nullptr, hipMemcpy(cnt, cnt_host, (size_t)n_waves * 64 * sizeof(int32_t), hipMemcpyHostToDevice));
    T2D_HIP(nullptr, hipMemset(out, 0xff, (size_t)n_waves * 65 * sizeof(int32_t)));   // (-1: a word the kernel did not write shows)
    T2D_HIP(nullptr, t2d::launch_wave_scan_probe(cnt, out, n_waves));
    T2D_HIP(nullptr, hipDeviceSynchronize());
    std::vector<int32_t> h((size_t)n_waves * 65);
    T2D_HIP(nullptr, hipMemcpy(h.data(), out, h.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    for (int w = 0; w < n_waves; ++w) {
        for (int l = 0; l < 64; ++l) off_host[64 * w + l] = h[65 * (size_t)w + l];
        total_host[w] = h[65 * (size_t)w + 64];
    }
    return T2D_OK;
}
#endif
#ifdef T2D_DEBUG_HOOKS   // include/t2d_debug.h: libt2d_hip_debug.so only
int t2d_debug_chain_fault(t2d_pool* p, int32_t kind) {
    if (!p) return T2D_ERR_INVALID;
    if (kind < 0 || kind > 3)
        return fail(p, T2D_ERR_INVALID, "fault kind: 0 none, 1 foreign XCC id at step 1, 2 a hand-off that never comes, 3 foreign XCC id at step 0");
    p->chain_fault = (uint32_t)kind;
    return T2D_OK;
}
#endif

#ifdef T2D_DEBUG_HOOKS   // include/t2d_debug.h: libt2d_hip_debug.so only
// placement of the step launch (include/t2d_debug.h): a permutation of its workgroups + a wave rotation per workgroup
int t2d_debug_set_step_placement(t2d_pool* p, const uint32_t* map_host, int32_t n_workgroups) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    if (!map_host || n_workgroups <= 0) {   // back to the identity
        p->v.wgmap = nullptr;
        return T2D_OK;
    }
    const int epb = p->v.geo_layout.epb > 0 ? p->v.geo_layout.epb : 1;
    const int n_blocks = (p->v.n_env + epb - 1) / epb;
    if (n_workgroups != n_blocks) return fail(p, T2D_ERR_INVALID, "placement map must have one entry per workgroup of the step launch");
    if (n_blocks > 65536) return fail(p, T2D_ERR_INVALID, "placement map: at most 65536 workgroups");   // 16-bit workgroup ids
    std::vector<uint8_t> seen((size_t)n_blocks, 0);
    for (int b = 0; b < n_blocks; ++b) {   // a permutation of the workgroups, rotations 0..3
        const uint32_t g = map_host[b] & 0xffffu, r = map_host[b] >> 16;
        if (g >= (uint32_t)n_blocks || r > 3u || seen[g]) return fail(p, T2D_ERR_INVALID, "placement map is not a permutation with rotations 0..3");
        seen[g] = 1;
    }
    if (!p->d_wgmap) T2D_HIP(p, p->d_wgmap.alloc(65536));
    T2D_HIP(p, hipMemcpy(p->d_wgmap, map_host, sizeof(uint32_t) * (size_t)n_blocks, hipMemcpyHostToDevice));
    p->v.wgmap = p->d_wgmap;
    return T2D_OK;
}
#endif

// capacity planning: resident workgroups per CU of the fused step kernel for this pool's geometry, and its LDS bytes per
// workgroup -- the regression guard of tests/test_gpu_api.py
int t2d_step_occupancy(t2d_pool* p, int32_t* blocks_per_cu, int64_t* lds_bytes, int64_t* geometry_bytes_per_launch) {
    if (!p || !blocks_per_cu || !lds_bytes) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    int b = 0;
    size_t l = 0;
    T2D_HIP(p, t2d::step_occupancy(p->v, &b, &l));
    *blocks_per_cu = b;
    *lds_bytes = (int64_t)l;
    if (geometry_bytes_per_launch) {   // the packed records every workgroup of a step launch stages into LDS
        const int epb = p->v.geo_layout.epb > 0 ? p->v.geo_layout.epb : 1;
        const int64_t n_blocks = (p->v.n_env + epb - 1) / epb;
        *geometry_bytes_per_launch = p->v.geo ? n_blocks * (int64_t)p->v.geo_layout.stride * 4 : 0;
    }
    return T2D_OK;
}

// a HIP stream of the library's own making (hipStreamNonBlocking, given priority: 0 = default, negative = higher): env groups
// on streams that do not come out of the caller's framework pool
int t2d_stream_create(int32_t device_id, int32_t priority, void** out_stream) {
    if (!out_stream) return T2D_ERR_INVALID;
    hipStream_t s = nullptr;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithPriority(&s, hipStreamNonBlocking, priority) != hipSuccess) {
        (void)hipGetLastError();
        return T2D_ERR_HIP;
    }
    *out_stream = s;
    return T2D_OK;
}
int t2d_stream_destroy(void* stream) {
    return hipStreamDestroy((hipStream_t)stream) == hipSuccess ? T2D_OK : T2D_ERR_HIP;
}

int t2d_get_field(t2d_pool* p, int32_t f, void** dev_ptr, size_t* nbytes) {
    if (!p) return T2D_ERR_INVALID;
    if (f < 0 || f >= T2D_F_COUNT || !dev_ptr) return fail(p, T2D_ERR_INVALID, "bad field id");
    *dev_ptr = p->field_ptr[f];
    if (nbytes) *nbytes = p->field_bytes[f];
    return T2D_OK;
}

int t2d_download(t2d_pool* p, int32_t f, void* host_dst, size_t nbytes) {
    if (!p) return T2D_ERR_INVALID;
    if (f < 0 || f >= T2D_F_COUNT || !host_dst || nbytes != p->field_bytes[f])
        return fail(p, T2D_ERR_INVALID, "bad field id / size (expected " +
                                            std::to_string(f >= 0 && f < T2D_F_COUNT ? p->field_bytes[f] : 0) + " bytes)");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    if (p->chain_failed || p->scene_commit_failed || p->trackgen_failed) return report_chain_failure(p);
    T2D_HIP(p, hipMemcpy(host_dst, p->field_ptr[f], nbytes, hipMemcpyDeviceToHost));
    return T2D_OK;
}

int t2d_upload(t2d_pool* p, int32_t f, const void* host_src, size_t nbytes) {
    if (!p) return T2D_ERR_INVALID;
    if (f < 0 || f >= T2D_F_COUNT || !host_src || nbytes != p->field_bytes[f])
        return fail(p, T2D_ERR_INVALID, "bad field id / size");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    T2D_HIP(p, hipMemcpy(p->field_ptr[f], host_src, nbytes, hipMemcpyHostToDevice));
    // an ids column written by the caller: which types are in use is no longer known -- every row of the table counts (the
    // integrator's single-model / four-per-lane instantiations are chosen from this set: t2d_integrate)
    if (f == T2D_F_IDS) p->types_used = ~0u;
    if (f == T2D_F_APPLIED0) p->applied_spans_restart = false;   // (the caller's accel_last for t2d_pursuit_actions, as written)
    // actions uploaded into the pool's own fields are the actions from now on: a binding to caller-owned device memory
    // (t2d_bind_actions) ends here, or the kernels would keep reading the caller's stale tensors
    if (f == T2D_F_ACT0 || f == T2D_F_ACT1) {
        p->v.act0 = (const float*)p->field_ptr[T2D_F_ACT0];
        p->v.act1 = (const float*)p->field_ptr[T2D_F_ACT1];
        p->v.act_stride = 1;
        p->act_extent = 0;
        p->act_in_frame = false;
        refresh_idm_view(p);
    }
    return T2D_OK;
}

int t2d_sync(t2d_pool* p) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    if (p->chain_failed || p->scene_commit_failed || p->trackgen_failed) return report_chain_failure(p);
    return T2D_OK;
}

// ---- the Gym-API host path (include/t2d.h: t2d_frame_config / t2d_step_host / t2d_frame_fetch) -------------------------------
static void frame_release(t2d_pool* p) {
    // the staging buffers go: a pool whose actions are the ones t2d_step_host staged there falls back to its own action
    // fields (what t2d_step / t2d_step_n / t2d_step_host(NULL) read from now on), never to freed memory
    if (p->act_in_frame) {
        p->v.act0 = (const float*)p->field_ptr[T2D_F_ACT0];
        p->v.act1 = (const float*)p->field_ptr[T2D_F_ACT1];
        p->v.act_stride = 1;
        p->act_extent = 0;
        p->act_in_frame = false;
        refresh_idm_view(p);
    }
    p->d_frame = {};
    p->d_actions = {};
    for (auto& h : p->h_frame) h = {};
    p->h_actions = {};
    p->frame_sections = 0;
    p->n_host_frames = 0;
    p->frame_layout = t2d_frame_layout{};
}

int t2d_frame_config(t2d_pool* p, uint32_t sections, int32_t n_host_frames, t2d_frame_layout* layout) {
    if (!p) return T2D_ERR_INVALID;
    if (n_host_frames < 1 || n_host_frames > T2D_MAX_HOST_FRAMES) return fail(p, T2D_ERR_INVALID, "need 1..16 host frames");
    if (sections & ~(T2D_FRAME_LIDAR | T2D_FRAME_TARGET | T2D_FRAME_ZEROCOPY)) return fail(p, T2D_ERR_INVALID, "unknown frame section bits");
    if ((sections & T2D_FRAME_LIDAR) && !p->lidar_on)
        return fail(p, T2D_ERR_STATE, "t2d_lidar_config must precede a frame with a lidar section");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    const size_t E = (size_t)p->v.n_env;
    t2d_frame_layout L{};
    size_t total = 256;   // header
    auto section = [&](size_t bytes) {
        const size_t off = total;
        total += (bytes + 255) & ~(size_t)255;
        return (int64_t)off;
    };
    L.off_rel = section(E * 3 * sizeof(double));
    L.off_obs = section(E * 6 * sizeof(float));
    L.off_reward = section(E * 4);
    L.off_status = section(E * 4);
    L.off_iou = section(E * 4);
    L.off_frame_ms = section(E * 4);
    L.off_cnt_step = section(E * 4);
    L.off_episode = section(E * 4);
    L.off_target = L.off_target_heading = L.off_lidar = -1;
    if (sections & T2D_FRAME_TARGET) {
        L.off_target_heading = section(E * sizeof(double));
        L.off_target = section(E * 8 * sizeof(float));
    }
    L.n_env = p->v.n_env;
    L.n_beams = 0;
    if (sections & T2D_FRAME_LIDAR) {
        L.n_beams = p->lidar.n_beams;
        L.off_lidar = section(E * (size_t)L.n_beams * sizeof(float));
    }
    L.bytes = (int64_t)total;
    // the same configuration again (every VecParkingEnv.reset asks): keep the frames -- a caller may still hold views of them
    if ((p->frame_sections & 0x7fffffffu) == sections && (p->frame_sections & 0x80000000u) && p->n_host_frames == n_host_frames &&
        memcmp(&p->frame_layout, &L, sizeof L) == 0) {
        if (layout) *layout = L;
        return T2D_OK;
    }
    frame_release(p);
    const unsigned host_flags = hipHostMallocMapped | hipHostMallocCoherent;
    for (int k = 0; k < n_host_frames; ++k) {
        T2D_HIP(p, p->h_frame[k].alloc(total, host_flags));
        memset(p->h_frame[k], 0, total);
    }
    p->n_host_frames = n_host_frames;
    const size_t act_bytes = (size_t)p->v.N * 2 * sizeof(float);
    T2D_HIP(p, p->h_actions.alloc((size_t)p->v.N * 2, host_flags));
    memset(p->h_actions, 0, act_bytes);
    if (!(sections & T2D_FRAME_ZEROCOPY)) {
        T2D_HIP(p, p->d_frame.alloc_zeroed(total));
        T2D_HIP(p, p->d_actions.alloc_zeroed((size_t)p->v.N * 2));
    }
    p->frame_sections = sections | 0x80000000u;   // (configured, whatever the section bits)
    p->frame_layout = L;
    p->frame_turn = 0;
    if (layout) *layout = L;
    return T2D_OK;
}

int t2d_set_target_headings(t2d_pool* p, const double* heading_host) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    return dev_replace(p, &p->d_target_heading, heading_host, heading_host ? (size_t)p->v.n_env : 0);
}

// scan (optional) + pack + fetch of the current state on `s`; returns with the host frame filled
static int frame_finish(t2d_pool* p, hipStream_t s, int frame_index, const void** frame_host) {
    const t2d_frame_layout& L = p->frame_layout;
    const bool zero_copy = (p->frame_sections & T2D_FRAME_ZEROCOPY) != 0;
    if (frame_index < 0) {
        frame_index = p->frame_turn;
        p->frame_turn = (p->frame_turn + 1) % p->n_host_frames;
    }
    char* host = p->h_frame[frame_index];
    char* dev_out = p->d_frame;
    if (zero_copy) T2D_HIP(p, hipHostGetDevicePointer((void**)&dev_out, host, 0));
    int rc;
    if (L.off_lidar >= 0) {
        if (!p->lidar_on || p->lidar.n_beams != L.n_beams)
            return fail(p, T2D_ERR_STATE, "the lidar configuration changed: call t2d_frame_config again");
        if ((rc = t2d_lidar_scan(p, reinterpret_cast<float*>(dev_out + L.off_lidar), s))) return rc;
    }
    t2d::FrameView fv{};
    fv.out = dev_out;
    fv.lay = L;
    fv.target_heading = p->scene_mode ? p->scene.live.target_heading : p->d_target_heading;
    fv.target_quads = p->scene_mode ? p->scene.live.target : nullptr;
    fv.episode = p->scene_mode ? p->scene.episode : nullptr;
    fv.commit_err = p->scene_mode && p->scene_regen ? p->scene.commit_err : nullptr;
    fv.step_count = (uint32_t)p->step_count;
    fv.ego_index = p->status_cfg.ego_index;
    touch(p, s);
    T2D_HIP(p, t2d::launch_frame_pack(p->v, fv, s));
    if (!zero_copy) T2D_HIP(p, hipMemcpyAsync(host, p->d_frame, (size_t)L.bytes, hipMemcpyDeviceToHost, s));
    T2D_HIP(p, hipStreamSynchronize(s));
    // `s` is drained: drop it from the streams a later quiesce has to wait for
    for (int k = 0; k < p->n_live_streams; ++k)
        if (p->live_streams[k] == s) {
            p->live_streams[k] = p->live_streams[--p->n_live_streams];
            break;
        }
    if (frame_host) *frame_host = host;
    if (fv.commit_err && reinterpret_cast<const uint32_t*>(host)[1]) {   // (what quiesce would have found with a blocking copy)
        (void)hipMemset(p->scene.commit_err, 0, sizeof(uint32_t));
        p->scene_commit_failed = true;
    }
    if (p->n_live_streams == 0 && !p->live_overflow && !p->chain_used) p->scene_commit_used = false;
    if (p->scene_commit_failed) return report_chain_failure(p);
    return T2D_OK;
}

int t2d_step_host(t2d_pool* p, const float* actions_host, const float* action_box, int32_t interval_ms, void* hip_stream,
                  int32_t frame_index, const void** frame_host) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->frame_sections) return fail(p, T2D_ERR_STATE, "t2d_frame_config must precede t2d_step_host");
    if (frame_index >= p->n_host_frames) return fail(p, T2D_ERR_INVALID, "frame_index out of range");
    if (interval_ms > 0)   // (ahead of the staging: a refused step stages nothing)
        if (int rc0 = replay_check(p, interval_ms)) return rc0;
    T2D_HIP(p, hipSetDevice(p->device));
    hipStream_t s = (hipStream_t)hip_stream;
    if (actions_host) {
        const size_t act_bytes = (size_t)p->v.N * 2 * sizeof(float);
        const bool in_place = actions_host == p->h_actions;   // the caller filled the pool's own pinned buffer (t2d_host_action_buffer)
        if (action_box) {   // Box.contains for every row, in the pass that stages the actions
            const float lo0 = action_box[0], hi0 = action_box[1], lo1 = action_box[2], hi1 = action_box[3];
            float* dst = p->h_actions;
            int ok = 1;
            // the verdict first, the copy only behind it: rejected rows (NaN included) never reach the staging buffer, which
            // in zero-copy mode IS what the previous call's binding reads -- a t2d_step after an InvalidAction steps with the
            // last accepted actions (a caller that filled the pool's own buffer in place has overwritten them itself)
            for (size_t i = 0, n = (size_t)p->v.N; i < n; ++i) {
                const float a = actions_host[2 * i], b = actions_host[2 * i + 1];
                ok &= (int)(a >= lo0) & (int)(a <= hi0) & (int)(b >= lo1) & (int)(b <= hi1);
            }
            if (ok && !in_place) memcpy(dst, actions_host, act_bytes);
            if (!ok) {
                size_t bad = 0;
                for (size_t n = (size_t)p->v.N; bad < n; ++bad) {
                    const float a = actions_host[2 * bad], b = actions_host[2 * bad + 1];
                    if (!(a >= lo0 && a <= hi0 && b >= lo1 && b <= hi1)) break;
                }
                return fail(p, T2D_ERR_ACTION, "action row " + std::to_string(bad) + " is not in the action space");
            }
        } else if (!in_place) {
            memcpy(p->h_actions, actions_host, act_bytes);
        }
        const float* dev_act = p->d_actions;
        if (p->frame_sections & T2D_FRAME_ZEROCOPY) {
            T2D_HIP(p, hipHostGetDevicePointer((void**)&dev_act, p->h_actions, 0));
        } else {
            touch(p, s);
            T2D_HIP(p, hipMemcpyAsync(p->d_actions, p->h_actions, act_bytes, hipMemcpyHostToDevice, s));
        }
        // (steering, accel) per participant: act0 (accel) = element 1, act1 (steering) = element 0, stride 2
        p->v.act0 = dev_act + 1;
        p->v.act1 = dev_act;
        p->v.act_stride = 2;
        p->act_extent = 0;
        p->act_in_frame = true;
        refresh_idm_view(p);
    }
    int rc = t2d_step(p, interval_ms, hip_stream);
    if (rc != T2D_OK) return rc;
    return frame_finish(p, s, frame_index, frame_host);
}

int t2d_host_action_buffer(t2d_pool* p, float** actions_host) {
    if (!p || !actions_host) return T2D_ERR_INVALID;
    if (!p->frame_sections) return fail(p, T2D_ERR_STATE, "t2d_frame_config must precede t2d_host_action_buffer");
    *actions_host = p->h_actions;
    return T2D_OK;
}

int t2d_frame_fetch(t2d_pool* p, void* hip_stream, int32_t frame_index, const void** frame_host) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->frame_sections) return fail(p, T2D_ERR_STATE, "t2d_frame_config must precede t2d_frame_fetch");
    if (frame_index >= p->n_host_frames) return fail(p, T2D_ERR_INVALID, "frame_index out of range");
    if (!p->have_params || !p->have_reset) return fail(p, T2D_ERR_STATE, "t2d_reset must precede t2d_frame_fetch");
    T2D_HIP(p, hipSetDevice(p->device));
    return frame_finish(p, (hipStream_t)hip_stream, frame_index, frame_host);
}

int t2d_lidar_config(t2d_pool* p, int32_t n_beams, float max_range, int32_t include_participants,
                     const double* beam_sin, const double* beam_cos) {
    if (!p) return T2D_ERR_INVALID;
    if (n_beams < 1 || n_beams > 4096 || !(max_range > 0.0f))
        return fail(p, T2D_ERR_INVALID, "need 1 <= n_beams <= 4096 and max_range > 0");
    if ((beam_sin == nullptr) != (beam_cos == nullptr)) return fail(p, T2D_ERR_INVALID, "pass both beam tables or neither");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    std::vector<double> bs(n_beams), bc(n_beams);
    bool regular = true;   // the beams stand at k * 2 pi / n_beams (what t2d_rs_config builds its obstacle chain on)
    for (int k = 0; k < n_beams; ++k) {
        if (beam_sin) {
            bs[k] = beam_sin[k];
            bc[k] = beam_cos[k];
            const double th = (double)k * ((2.0 * 3.141592653589793) / (double)n_beams);
            regular = regular && fabs(bs[k] - sin(th)) <= 1e-9 && fabs(bc[k] - cos(th)) <= 1e-9;
        } else {  // linspace(0, 2 pi, n, endpoint=False) = k * (2 pi / n)
            const double th = (double)k * ((2.0 * 3.141592653589793) / (double)n_beams);
            bs[k] = sin(th);
            bc[k] = cos(th);
        }
    }
    int rc;
    {   // what the determinant solve needs of a beam, once per beam instead of once per candidate (same expressions as
        // lidar.py:161-162, 201-213: a, b of the beam's line, its end point (lx, ly) = (cos, sin) * R widened by 1e-8)
        const double R = (double)max_range, tz = 1e-8;
        std::vector<double> pre(6 * (size_t)n_beams);
        for (int k = 0; k < n_beams; ++k) {
            const double lx = bc[k] * R, ly = bs[k] * R;
            const double mx = tz > lx ? tz : lx, nx = -tz < lx ? -tz : lx;
            const double my = tz > ly ? tz : ly, ny = -tz < ly ? -tz : ly;
            double* r = &pre[6 * (size_t)k];
            r[0] = bs[k]; r[1] = -bc[k]; r[2] = mx + tz; r[3] = nx - tz; r[4] = my + tz; r[5] = ny - tz;
        }
        if ((rc = dev_replace(p, &p->d_beam_sin, pre.data(), pre.size()))) return rc;
    }
    // the scan buffer is kept when the beam count is unchanged (every VecParkingEnv.reset reconfigures the lidar): a
    // zero-copy view a caller took with t2d_get_field stays valid until the size really changes
    const size_t lidar_bytes = (size_t)p->v.n_env * n_beams * sizeof(float);
    if (!p->field_ptr[T2D_F_LIDAR] || p->field_bytes[T2D_F_LIDAR] != lidar_bytes) {
        p->field_ptr[T2D_F_LIDAR] = nullptr;   // (a failed allocation leaves the field empty: no pointer, no size)
        p->field_bytes[T2D_F_LIDAR] = 0;
        T2D_HIP(p, p->field_buf[T2D_F_LIDAR].alloc(lidar_bytes));
        p->field_ptr[T2D_F_LIDAR] = p->field_buf[T2D_F_LIDAR];
        p->field_bytes[T2D_F_LIDAR] = lidar_bytes;
    }
    T2D_HIP(p, hipMemset(p->field_ptr[T2D_F_LIDAR], 0, lidar_bytes));
    // the all-participants buffer follows the configuration: a new beam count drops it, the next NULL-destination
    // t2d_lidar_scan_all allocates it again (a view taken with t2d_lidar_all_buffer stays valid while the size does)
    if (p->d_lidar_all && p->d_lidar_all.bytes() != lidar_bytes * (size_t)p->v.A) T2D_HIP(p, p->d_lidar_all.reset());
    p->lidar.beam_pre = p->d_beam_sin;
    p->lidar.max_range = (double)max_range;
    p->lidar.n_beams = n_beams;
    p->lidar.include_participants = include_participants != 0;
    p->lidar_on = true;
    p->lidar_regular = regular;
    rc = rebuild_lidar_geo(p);
    if (rc != T2D_OK) return rc;
    return T2D_OK;
}

int t2d_lidar_scan(t2d_pool* p, float* out_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->lidar_on) return fail(p, T2D_ERR_STATE, "t2d_lidar_config must precede t2d_lidar_scan");
    if (!p->have_params || !p->have_reset) return fail(p, T2D_ERR_STATE, "t2d_reset must precede t2d_lidar_scan");
    p->lidar.ego_index = p->status_cfg.ego_index;
    hipStream_t s = (hipStream_t)hip_stream;
    int rc;
    if ((rc = lidar_fits(p))) return rc;   // (a configuration t2d_lidar_config refused: no launch)
    touch(p, s);
    if ((rc = record_event(p, 3, s, true))) return rc;
    T2D_HIP(p, t2d::launch_lidar(p->v, p->lidar, out_dev ? out_dev : (float*)p->field_ptr[T2D_F_LIDAR], s));
    return record_event(p, 3, s, false);
}

int t2d_lidar_scan_all(t2d_pool* p, float* out_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->lidar_on) return fail(p, T2D_ERR_STATE, "t2d_lidar_config must precede t2d_lidar_scan_all");
    if (!p->have_params || !p->have_reset) return fail(p, T2D_ERR_STATE, "t2d_reset must precede t2d_lidar_scan_all");
    hipStream_t s = (hipStream_t)hip_stream;
    int rc;
    if ((rc = lidar_fits(p))) return rc;
    if (!out_dev && !p->d_lidar_all) {   // first use of the pool's own buffer (or the first after a new beam count)
        T2D_HIP(p, hipSetDevice(p->device));
        T2D_HIP(p, p->d_lidar_all.alloc((size_t)p->v.n_env * p->v.A * p->lidar.n_beams));
    }
    touch(p, s);
    if ((rc = record_event(p, 8, s, true))) return rc;
    T2D_HIP(p, t2d::launch_lidar_all(p->v, p->lidar, out_dev ? out_dev : p->d_lidar_all, s));
    return record_event(p, 8, s, false);
}

int t2d_lidar_all_buffer(t2d_pool* p, void** dev_ptr, size_t* nbytes) {
    if (!p) return T2D_ERR_INVALID;
    if (!dev_ptr || !nbytes) return fail(p, T2D_ERR_INVALID, "null output");
    if (!p->d_lidar_all)
        return fail(p, T2D_ERR_STATE, "a t2d_lidar_scan_all with a NULL destination must precede t2d_lidar_all_buffer");
    *dev_ptr = p->d_lidar_all;
    *nbytes = p->d_lidar_all.bytes();
    return T2D_OK;
}

int t2d_rs_config(t2d_pool* p, const t2d_rs_params* cfg, const float* vehicle_base_host) {
    if (!p) return T2D_ERR_INVALID;
    if (!cfg) return fail(p, T2D_ERR_INVALID, "t2d_rs_config: null configuration");
    const double vals[9] = {cfg->radius, cfg->center_shift, cfg->half_length, cfg->half_width, cfg->distance_tolerance,
                            cfg->threshold_distance, cfg->sample_step, cfg->length_ratio, cfg->edge_tolerance};
    for (double v : vals)
        if (!std::isfinite(v)) return fail(p, T2D_ERR_INVALID, "t2d_rs_config: every value must be finite");
    if (!(cfg->radius > 0.0 && cfg->half_length > 0.0 && cfg->half_width > 0.0 && cfg->sample_step > 0.0 && cfg->length_ratio >= 1.0 &&
          cfg->distance_tolerance >= 0.0 && cfg->threshold_distance >= 0.0 && cfg->edge_tolerance >= 0.0))
        return fail(p, T2D_ERR_INVALID, "t2d_rs_config: need radius, half_length, half_width, sample_step > 0, length_ratio >= 1 "
                                        "and tolerances / threshold >= 0");
    if (!p->lidar_on) return fail(p, T2D_ERR_STATE, "t2d_lidar_config must precede t2d_rs_config");
    if (!p->lidar_regular)
        return fail(p, T2D_ERR_STATE, "t2d_rs_config: the lidar's beam tables are not the angles k * 2 pi / n_beams the planner's chain is built on");
    const int n = p->lidar.n_beams;
    if (n > T2D_RS_MAX_BEAMS) return fail(p, T2D_ERR_INVALID, "t2d_rs_config: the planner takes at most 1024 beams");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    // per beam: cos, sin of np.arange(n) * np.pi / n * 2 (cell 9 :164) and vehicle_base (init_vehicle_base :23-44)
    std::vector<double> tab(3 * (size_t)n);
    for (int k = 0; k < n; ++k) {
        const double th = (double)k * 3.141592653589793 / (double)n * 2.0;
        const double cs = cos(th), sn = sin(th);
        tab[3 * (size_t)k] = cs;
        tab[3 * (size_t)k + 1] = sn;
        if (vehicle_base_host) {
            tab[3 * (size_t)k + 2] = (double)vehicle_base_host[k];
        } else {   // the ray from the centre leaves the box through the nearer of the two pairs of sides
            const double dx = fabs(cs) > 0.0 ? cfg->half_length / fabs(cs) : INFINITY;
            const double dy = fabs(sn) > 0.0 ? cfg->half_width / fabs(sn) : INFINITY;
            tab[3 * (size_t)k + 2] = dx < dy ? dx : dy;
        }
        if (!std::isfinite(tab[3 * (size_t)k + 2])) return fail(p, T2D_ERR_INVALID, "t2d_rs_config: vehicle_base must be finite");
    }
    int rc;
    if ((rc = dev_replace(p, &p->d_rs_beam_tab, tab.data(), tab.size()))) return rc;
    if (!p->d_rs_plan) T2D_HIP(p, p->d_rs_plan.alloc_zeroed((size_t)p->v.n_env));
    p->rs.cfg = *cfg;
    p->rs.lidar_range = p->lidar.max_range;
    p->rs.beam_tab = p->d_rs_beam_tab;
    p->rs.n_beams = n;
    p->rs_on = true;
    return T2D_OK;
}

int t2d_rs_plan(t2d_pool* p, const float* lidar_dev, t2d_rs_plan_record* out_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->rs_on) return fail(p, T2D_ERR_STATE, "t2d_rs_config must precede t2d_rs_plan");
    if (!p->lidar_on || !p->lidar_regular || p->lidar.n_beams != p->rs.n_beams || p->lidar.max_range != p->rs.lidar_range)
        return fail(p, T2D_ERR_STATE, "the lidar configuration changed: call t2d_rs_config again");
    if (!p->have_params || !p->have_reset) return fail(p, T2D_ERR_STATE, "t2d_reset must precede t2d_rs_plan");
    if (reinterpret_cast<uintptr_t>(out_dev) & 7u) return fail(p, T2D_ERR_INVALID, "t2d_rs_plan: out_dev must be 8-byte aligned");
    t2d::RsPlanView rv = p->rs;
    if (p->scene_mode) {
        rv.target_xy = nullptr;
        rv.target_quads = p->scene.live.target;
        rv.target_heading = p->scene.live.target_heading;
    } else {
        rv.target_xy = p->have_target ? p->d_target_xy : nullptr;
        rv.target_quads = nullptr;
        rv.target_heading = p->d_target_heading;
    }
    if ((!rv.target_xy && !rv.target_quads) || !rv.target_heading)
        return fail(p, T2D_ERR_STATE, "t2d_rs_plan needs target areas and target headings");
    rv.ego_index = p->status_cfg.ego_index;
    hipStream_t s = (hipStream_t)hip_stream;
    int rc;
    touch(p, s);
    if ((rc = record_event(p, T2D_PROFILE_RS_PLAN, s, true))) return rc;
    T2D_HIP(p, t2d::launch_rs_plan(p->v, rv, lidar_dev ? lidar_dev : (const float*)p->field_ptr[T2D_F_LIDAR],
                                   out_dev ? out_dev : p->d_rs_plan, s));
    return record_event(p, T2D_PROFILE_RS_PLAN, s, false);
}

// the pool's own records of an installed source (the t2d_*_buffers entry points): where they are and how many bytes
static int own_records(t2d_pool* p, bool on, const char* need, void* records, size_t bytes, void** records_dev, size_t* nbytes) {
    if (!records_dev || !nbytes) return fail(p, T2D_ERR_INVALID, "null output");
    if (!on) return fail(p, T2D_ERR_STATE, need);
    *records_dev = records;
    *nbytes = bytes;
    return T2D_OK;
}

int t2d_rs_plan_buffers(t2d_pool* p, void** dev_ptr, size_t* nbytes) {
    if (!p) return T2D_ERR_INVALID;
    return own_records(p, p->rs_on, "t2d_rs_config must precede t2d_rs_plan_buffers", p->d_rs_plan.get(),
                       (size_t)p->v.n_env * sizeof(t2d_rs_plan_record), dev_ptr, nbytes);
}

static int rs_follow_clear(t2d_pool* p) {
    const size_t E = (size_t)p->v.n_env;
    T2D_HIP(p, hipMemset(p->rs_follow.f64, 0, (size_t)t2d::kRfF64Rows * E * sizeof(double)));
    T2D_HIP(p, hipMemset(p->rs_follow.i32, 0, (size_t)t2d::kRfI32Rows * E * sizeof(int32_t)));
    T2D_HIP(p, hipMemset(p->d_rs_follow_rec, 0, E * sizeof(t2d_rs_follow_record)));
    std::vector<double> inf(E, INFINITY);   // distance_record is empty
    T2D_HIP(p, hipMemcpy(p->rs_follow.f64 + (size_t)t2d::kRfLast * E, inf.data(), E * sizeof(double), hipMemcpyHostToDevice));
    return T2D_OK;
}

int t2d_rs_follow_config(t2d_pool* p, const t2d_rs_follow_params* cfg) {
    if (!p) return T2D_ERR_INVALID;
    if (!cfg) return fail(p, T2D_ERR_INVALID, "t2d_rs_follow_config: null configuration");
    const double* vals = reinterpret_cast<const double*>(cfg);
    for (size_t k = 0; k < sizeof(*cfg) / sizeof(double); ++k)
        if (!std::isfinite(vals[k])) return fail(p, T2D_ERR_INVALID, "t2d_rs_follow_config: every value must be finite");
    if (!(cfg->radius > 0.0 && cfg->max_speed > 0.0 && cfg->max_acceleration > 0.0 && cfg->reach_radius > 0.0 &&
          cfg->rising_radius > 0.0 && cfg->steer_bound > 0.0 && cfg->accel_bound > 0.0))
        return fail(p, T2D_ERR_INVALID, "t2d_rs_follow_config: need radius, max_speed, max_acceleration, reach_radius, rising_radius, "
                                        "steer_bound, accel_bound > 0");
    if (!p->rs_on) return fail(p, T2D_ERR_STATE, "t2d_rs_config must precede t2d_rs_follow_config");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    const size_t E = (size_t)p->v.n_env;
    if (!p->d_rs_follow_f64) T2D_HIP(p, p->d_rs_follow_f64.alloc((size_t)t2d::kRfF64Rows * E));
    if (!p->d_rs_follow_i32) T2D_HIP(p, p->d_rs_follow_i32.alloc((size_t)t2d::kRfI32Rows * E));
    if (!p->d_rs_follow_rec) T2D_HIP(p, p->d_rs_follow_rec.alloc(E));
    p->rs_follow.f64 = p->d_rs_follow_f64;
    p->rs_follow.i32 = p->d_rs_follow_i32;
    int rc;
    if ((rc = rs_follow_clear(p))) return rc;
    p->rs_follow.cfg = *cfg;
    p->rs_follow_on = true;
    return T2D_OK;
}

int t2d_rs_follow(t2d_pool* p, const t2d_rs_plan_record* plan_dev, const float* act_in_dev, float* act_out_dev,
                  t2d_rs_follow_record* out_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->rs_follow_on) return fail(p, T2D_ERR_STATE, "t2d_rs_follow_config must precede t2d_rs_follow");
    if (!p->have_params || !p->have_reset) return fail(p, T2D_ERR_STATE, "t2d_reset must precede t2d_rs_follow");
    if (!act_out_dev) return fail(p, T2D_ERR_INVALID, "t2d_rs_follow: act_out_dev is required");
    if ((reinterpret_cast<uintptr_t>(out_dev) | reinterpret_cast<uintptr_t>(plan_dev)) & 7u)
        return fail(p, T2D_ERR_INVALID, "t2d_rs_follow: plan_dev and out_dev must be 8-byte aligned");
    t2d::RsFollowView fv = p->rs_follow;
    fv.ego_index = p->status_cfg.ego_index;
    hipStream_t s = (hipStream_t)hip_stream;
    int rc;
    touch(p, s);
    if ((rc = record_event(p, T2D_PROFILE_RS_FOLLOW, s, true))) return rc;
    T2D_HIP(p, t2d::launch_rs_follow(p->v, fv, plan_dev ? plan_dev : p->d_rs_plan, act_in_dev, act_out_dev,
                                     out_dev ? out_dev : p->d_rs_follow_rec, s));
    return record_event(p, T2D_PROFILE_RS_FOLLOW, s, false);
}

int t2d_rs_follow_reset(t2d_pool* p, const uint8_t* mask_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->rs_follow_on) return fail(p, T2D_ERR_STATE, "t2d_rs_follow_config must precede t2d_rs_follow_reset");
    hipStream_t s = (hipStream_t)hip_stream;
    touch(p, s);
    T2D_HIP(p, t2d::launch_rs_follow_reset(p->v, p->rs_follow, mask_dev, s));
    return T2D_OK;
}

int t2d_rs_follow_buffers(t2d_pool* p, void** records_dev, size_t* nbytes) {
    if (!p) return T2D_ERR_INVALID;
    return own_records(p, p->rs_follow_on, "t2d_rs_follow_config must precede t2d_rs_follow_buffers", p->d_rs_follow_rec.get(),
                       (size_t)p->v.n_env * sizeof(t2d_rs_follow_record), records_dev, nbytes);
}

// ---- scripted action sources: IDM (t2d_idm.hip), lane-keeping PID (t2d_pid.hip), pure pursuit and cruise / ACC (t2d_pursuit.hip)
// One order for the three setters: validate the host arguments, quiesce, check against the pool's state, stage every new device
// block in locals, move them in and fill the view.  A call that returns an error has changed nothing in the pool.  n_ctrl == 0
// uninstalls: quiesce, then the family's clear() -- flags, view and host copy gone, device blocks freed.
namespace {

constexpr int kCtrlNone = 255;
static_assert(T2D_IDM_NONE == kCtrlNone && T2D_PID_NONE == kCtrlNone && T2D_PURSUIT_NONE == kCtrlNone, "one 'no controller' id");

// The front of a setter: the arguments against the family's column count, the rows copied densely into `rows` with every row
// put to check_row(c, row) -- an empty string, or what is wrong with it -- and the range of ctrl_id.
int ctrl_front(t2d_pool* p, const std::string& who, int cols, const double* ctrl_rows, int n_ctrl, int row_stride, const uint8_t* ctrl_id,
               std::vector<double>& rows, const std::function<std::string(int, const double*)>& check_row) {
    if (!ctrl_rows || !ctrl_id || n_ctrl < 0 || n_ctrl >= kCtrlNone || row_stride < cols)
        return fail(p, T2D_ERR_INVALID, who + ": need 1..254 parameter sets of >= " + std::to_string(cols) +
                                            " columns and a controller id per participant");
    rows.resize((size_t)n_ctrl * cols);
    for (int c = 0; c < n_ctrl; ++c) {
        const double* r = ctrl_rows + (size_t)c * row_stride;
        std::copy(r, r + cols, rows.begin() + (size_t)c * cols);
        const std::string wrong = check_row(c, r);
        if (!wrong.empty()) return fail(p, T2D_ERR_INVALID, who + ": " + wrong + " (row " + std::to_string(c) + ")");
    }
    for (int i = 0; i < p->v.N; ++i)
        if (ctrl_id[i] != kCtrlNone && ctrl_id[i] >= n_ctrl)
            return fail(p, T2D_ERR_INVALID, who + ": ctrl_id[" + std::to_string(i) + "] = " + std::to_string((int)ctrl_id[i]) +
                                                " out of range");
    return T2D_OK;
}

// A participant has one controller: the first participant of `ctrl_id` that another installed family holds refuses the call.
int one_controller(t2d_pool* p, const std::string& who, const uint8_t* ctrl_id) {
    const struct {
        const char *setter, *name;
        bool on;
        const std::vector<uint8_t>& held;
    } families[] = {{"t2d_set_idm", "IDM", p->idm.on, p->idm.ctrl_host},
                    {"t2d_set_pid", "PID", p->pid.on, p->pid.ctrl_host},
                    {"t2d_set_pursuit", "pursuit", p->pursuit.on, p->pursuit.ctrl_host}};
    for (int i = 0; i < p->v.N; ++i)
        for (const auto& f : families)
            if (ctrl_id[i] != kCtrlNone && f.on && who != f.setter && f.held[i] != kCtrlNone)
                return fail(p, T2D_ERR_INVALID, who + ": participant " + std::to_string(i) + " is " + f.name + "-controlled (" +
                                                    f.setter + ")");
    return T2D_OK;
}

// The gate of t2d_pid_actions / t2d_pursuit_actions.  `lat_rows`: how the family words "a row steers" (null: none installed
// does); `state_wrong`: the family's own complaint about the pool's state, or null.
int actions_gate(t2d_pool* p, const std::string& who, const char* setter, bool on, const char* lat_rows, const char* state_wrong,
                 const float* act_out_dev, const void* record_dev) {
    if (!on) return fail(p, T2D_ERR_STATE, std::string(setter) + " must precede " + who);
    if (!p->have_params || !p->have_reset) return fail(p, T2D_ERR_STATE, "t2d_reset must precede " + who);
    if (p->route.kind == 2)
        return fail(p, T2D_ERR_STATE, who + " follows route sets (t2d_set_routes); trace routes are the installed kind");
    if (lat_rows && p->route.kind != 1)
        return fail(p, T2D_ERR_STATE, who + ": a row has " + lat_rows + " and no route set is installed (t2d_set_routes)");
    if (state_wrong) return fail(p, T2D_ERR_STATE, who + ": " + state_wrong);
    if (!act_out_dev) return fail(p, T2D_ERR_INVALID, who + ": act_out_dev is required");
    if (reinterpret_cast<uintptr_t>(record_dev) & 7u) return fail(p, T2D_ERR_INVALID, who + ": record_dev must be 8-byte aligned");
    return T2D_OK;
}

}  // namespace

int t2d_set_idm(t2d_pool* p, const double* ctrl_rows, int32_t n_ctrl, int32_t row_stride, const uint8_t* ctrl_id) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    if (n_ctrl == 0) {
        T2D_HIP(p, quiesce(p));   // (nothing in flight reads the blocks any more)
        const hipError_t e = p->idm.clear();
        refresh_idm_view(p);
        T2D_HIP(p, e);
        return T2D_OK;
    }
    const std::string who = "t2d_set_idm";
    std::vector<double> rows;
    int rc = ctrl_front(p, who, T2D_IDM_COLS, ctrl_rows, n_ctrl, row_stride, ctrl_id, rows, [](int, const double* r) -> std::string {
        // idm_controller.py divides by sqrt(max_acceleration * comfortable_deceleration) (:121)
        if (!(r[T2D_IDM_MAX_ACCEL] * r[T2D_IDM_COMF_DECEL] > 0.0)) return "max_acceleration * comfortable_deceleration must be positive";
        if (!(r[T2D_IDM_LANE_HALF_WIDTH] >= 0.0) || !(r[T2D_IDM_HORIZON] > 0.0)) return "lane_half_width >= 0 and horizon > 0 required";
        return "";
    });
    if (rc) return rc;
    T2D_HIP(p, quiesce(p));
    if ((rc = one_controller(p, who, ctrl_id))) return rc;
    const size_t N = (size_t)p->v.N;
    t2d::IdmFamily f;   // the new family whole; the installed one goes when nothing can fail any more
    if ((rc = dev_replace(p, &f.d_rows, rows.data(), rows.size()))) return rc;
    if ((rc = dev_replace(p, &f.d_ctrl, ctrl_id, N))) return rc;
    T2D_HIP(p, hipMemset(p->field_ptr[T2D_F_LEADER], 0xff, p->field_bytes[T2D_F_LEADER]));
    f.ctrl_host.assign(ctrl_id, ctrl_id + N);
    f.view = t2d::IdmView{f.d_rows, f.d_ctrl, (int32_t*)p->field_ptr[T2D_F_LEADER], n_ctrl};
    f.on = true;
    p->idm = std::move(f);
    refresh_idm_view(p);
    return T2D_OK;
}

int t2d_idm_actions(t2d_pool* p, const int32_t* forced_leader_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->idm.on) return fail(p, T2D_ERR_STATE, "t2d_set_idm must precede t2d_idm_actions");
    if (!p->have_reset) return fail(p, T2D_ERR_STATE, "t2d_reset must precede t2d_idm_actions");
    return idm_impl(p, (hipStream_t)hip_stream, forced_leader_dev);
}

int t2d_set_pid(t2d_pool* p, const double* ctrl_rows, int32_t n_ctrl, int32_t row_stride, const uint8_t* ctrl_id,
                const float* target_speed, const int32_t* idm_row) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    if (n_ctrl == 0) {
        T2D_HIP(p, quiesce(p));   // (nothing in flight reads the blocks any more)
        T2D_HIP(p, p->pid.clear());
        return T2D_OK;
    }
    const std::string who = "t2d_set_pid";
    std::vector<double> rows;
    std::vector<int> lon_of;
    bool any_lat = false;
    int rc = ctrl_front(p, who, T2D_PID_COLS, ctrl_rows, n_ctrl, row_stride, ctrl_id, rows, [&](int, const double* r) -> std::string {
        // pid_controller.py:87-102, comparison by comparison
        if (r[T2D_PID_DT] <= 0) return "dt must be positive";
        if (r[T2D_PID_MAX_STEERING] <= 0) return "max_steering must be positive";
        if (r[T2D_PID_MAX_ACCEL] <= 0) return "max_accel must be positive";
        if (r[T2D_PID_MIN_ACCEL] >= 0) return "min_accel must be negative (deceleration)";
        if (r[T2D_PID_MAX_ACCEL] <= r[T2D_PID_MIN_ACCEL]) return "max_accel must be greater than min_accel";
        if (r[T2D_PID_ALPHA] <= 0 || r[T2D_PID_ALPHA] > 1) return "derivative_filter_alpha must be in range (0, 1]";
        const double lat = r[T2D_PID_LAT_MODE], lon = r[T2D_PID_LON_MODE];
        if (!(lat == 0.0 || lat == 1.0 || lat == 2.0) || !(lon == 0.0 || lon == 1.0 || lon == 2.0 || lon == 3.0))
            return "lat_mode must be 0, 1 or 2 and lon_mode 0, 1, 2 or 3";
        lon_of.push_back((int)lon);
        any_lat = any_lat || lat != 0.0;
        return "";
    });
    if (rc) return rc;
    T2D_HIP(p, quiesce(p));
    if ((rc = one_controller(p, who, ctrl_id))) return rc;
    const int N = p->v.N;
    std::vector<float> ts(N, 0.f);
    if (target_speed) ts.assign(target_speed, target_speed + N);
    std::vector<int32_t> irow(N, 0);
    int idm_needed = 0;
    for (int i = 0; i < N; ++i) {
        if (ctrl_id[i] == kCtrlNone || lon_of[ctrl_id[i]] != 2) continue;
        if (!p->idm.on) return fail(p, T2D_ERR_STATE, who + ": lon_mode 2 needs the parameter sets of t2d_set_idm");
        irow[i] = idm_row ? idm_row[i] : 0;
        if (irow[i] < 0 || irow[i] >= p->idm.view.n_ctrl)
            return fail(p, T2D_ERR_INVALID, who + ": idm_row[" + std::to_string(i) + "] = " + std::to_string(irow[i]) +
                                                " outside the installed IDM rows");
        idm_needed = std::max(idm_needed, irow[i] + 1);
    }
    t2d::PidFamily f;   // the new family whole; the installed one goes when nothing can fail any more
    if ((rc = dev_replace(p, &f.d_rows, rows.data(), rows.size()))) return rc;
    if ((rc = dev_replace(p, &f.d_ctrl, ctrl_id, (size_t)N))) return rc;
    if ((rc = dev_replace(p, &f.d_target, ts.data(), (size_t)N))) return rc;
    if ((rc = dev_replace(p, &f.d_idm_row, irow.data(), (size_t)N))) return rc;
    T2D_HIP(p, f.d_state.alloc_zeroed((size_t)T2D_PID_STATE_WORDS * N));
    T2D_HIP(p, f.d_rec.alloc_zeroed((size_t)N));
    f.ctrl_host.assign(ctrl_id, ctrl_id + N);
    f.any_lat = any_lat;
    f.idm_rows_needed = idm_needed;
    // (idm_rows / n_idm: whatever t2d_set_idm has installed when a call is made -- t2d_pid_actions fills them in)
    f.view = t2d::PidView{f.d_rows, f.d_ctrl, f.d_target, f.d_idm_row, f.d_state, nullptr, n_ctrl, 0, idm_needed > 0};
    f.on = true;
    p->pid = std::move(f);
    return T2D_OK;
}

int t2d_pid_actions(t2d_pool* p, const float* act_in_dev, float* act_out_dev, t2d_pid_record* record_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    const bool rows_gone = p->pid.idm_rows_needed > 0 && (!p->idm.on || p->idm.view.n_ctrl < p->pid.idm_rows_needed);
    int rc = actions_gate(p, "t2d_pid_actions", "t2d_set_pid", p->pid.on, p->pid.any_lat ? "lat_mode != 0" : nullptr,
                          rows_gone ? "the IDM parameter sets lon_mode 2 was installed against are gone (t2d_set_idm)" : nullptr,
                          act_out_dev, record_dev);
    if (rc) return rc;
    t2d::PidView cv = p->pid.view;
    cv.idm_rows = p->idm.on ? p->idm.d_rows.get() : nullptr;
    cv.n_idm = p->idm.on ? p->idm.view.n_ctrl : 0;
    hipStream_t s = (hipStream_t)hip_stream;
    touch(p, s);
    if ((rc = record_event(p, T2D_PROFILE_PID, s, true))) return rc;
    T2D_HIP(p, t2d::launch_pid(p->v, cv, p->route, act_in_dev, act_out_dev, record_dev ? record_dev : p->pid.d_rec.get(), s));
    return record_event(p, T2D_PROFILE_PID, s, false);
}

int t2d_pid_reset(t2d_pool* p, const uint8_t* env_mask_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->pid.on) return fail(p, T2D_ERR_STATE, "t2d_set_pid must precede t2d_pid_reset");
    hipStream_t s = (hipStream_t)hip_stream;
    touch(p, s);
    T2D_HIP(p, t2d::launch_pid_reset(p->v, p->pid.view, env_mask_dev, s));
    return T2D_OK;
}

int t2d_pid_state(t2d_pool* p, double* state_host, int32_t write) {
    if (!p) return T2D_ERR_INVALID;
    if (!state_host) return fail(p, T2D_ERR_INVALID, "t2d_pid_state: null array");
    if (!p->pid.on) return fail(p, T2D_ERR_STATE, "t2d_set_pid must precede t2d_pid_state");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    const size_t N = (size_t)p->v.N;
    std::vector<double> soa((size_t)T2D_PID_STATE_WORDS * N);   // the device's layout: [word][participant]
    if (write) {
        for (size_t i = 0; i < N; ++i)
            for (int w = 0; w < T2D_PID_STATE_WORDS; ++w) soa[w * N + i] = state_host[i * T2D_PID_STATE_WORDS + w];
        T2D_HIP(p, hipMemcpy(p->pid.d_state, soa.data(), soa.size() * sizeof(double), hipMemcpyHostToDevice));
    } else {
        T2D_HIP(p, hipMemcpy(soa.data(), p->pid.d_state, soa.size() * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < N; ++i)
            for (int w = 0; w < T2D_PID_STATE_WORDS; ++w) state_host[i * T2D_PID_STATE_WORDS + w] = soa[w * N + i];
    }
    return T2D_OK;
}

int t2d_pid_buffers(t2d_pool* p, void** records_dev, size_t* nbytes) {
    if (!p) return T2D_ERR_INVALID;
    return own_records(p, p->pid.on, "t2d_set_pid must precede t2d_pid_buffers", p->pid.d_rec.get(),
                       (size_t)p->v.N * sizeof(t2d_pid_record), records_dev, nbytes);
}

int t2d_set_pursuit(t2d_pool* p, const double* ctrl_rows, int32_t n_ctrl, int32_t row_stride, const uint8_t* ctrl_id,
                    const float* target_speed) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    if (n_ctrl == 0) {
        T2D_HIP(p, quiesce(p));   // (nothing in flight reads the blocks any more)
        T2D_HIP(p, p->pursuit.clear());
        return T2D_OK;
    }
    const std::string who = "t2d_set_pursuit";
    std::vector<double> rows;
    std::vector<int> lon_of;
    bool any_lat = false, any_acc = false, any_last = false;
    int rc = ctrl_front(p, who, T2D_PURSUIT_COLS, ctrl_rows, n_ctrl, row_stride, ctrl_id, rows, [&](int, const double* r) -> std::string {
        for (int k = 0; k < T2D_PURSUIT_COLS; ++k) {
            const bool may = (k == T2D_PURSUIT_WHEEL_BASE && r[k] != r[k]) || (k == T2D_PURSUIT_HORIZON && r[k] == HUGE_VAL);
            if (!std::isfinite(r[k]) && !may) return "column " + std::to_string(k) + " is not finite";
        }
        // pure_pursuit_controller.py:31-32
        if (r[T2D_PURSUIT_MIN_PRE_AIMING] <= 0) return "min_pre_aiming_distance must be positive";
        const double lat = r[T2D_PURSUIT_LAT_MODE], lon = r[T2D_PURSUIT_LON_MODE];
        if (!(lat == 0.0 || lat == 1.0) || !(lon == 0.0 || lon == 1.0 || lon == 2.0)) return "lat_mode must be 0 or 1 and lon_mode 0, 1 or 2";
        lon_of.push_back((int)lon);
        any_lat = any_lat || lat == 1.0;
        any_acc = any_acc || lon == 1.0;
        any_last = any_last || lon != 2.0;
        return "";
    });
    if (rc) return rc;
    const int N = p->v.N;
    std::vector<float> ts(N, 0.f);
    if (target_speed) ts.assign(target_speed, target_speed + N);
    for (int i = 0; i < N; ++i)   // acceleration_controller.py:46-47 (the caller's acceleration needs no target speed)
        if (ctrl_id[i] != kCtrlNone && lon_of[ctrl_id[i]] != 2 && !(ts[i] >= 0))
            return fail(p, T2D_ERR_INVALID, who + ": target_speed[" + std::to_string(i) + "] must be non-negative");
    T2D_HIP(p, quiesce(p));
    if ((rc = one_controller(p, who, ctrl_id))) return rc;
    t2d::PursuitFamily f;   // the new family whole; the installed one goes when nothing can fail any more
    if ((rc = dev_replace(p, &f.d_rows, rows.data(), rows.size()))) return rc;
    if ((rc = dev_replace(p, &f.d_ctrl, ctrl_id, (size_t)N))) return rc;
    if ((rc = dev_replace(p, &f.d_target, ts.data(), (size_t)N))) return rc;
    T2D_HIP(p, f.d_rec.alloc_zeroed((size_t)N));
    f.ctrl_host.assign(ctrl_id, ctrl_id + N);
    f.any_lat = any_lat;
    f.any_last = any_last;
    f.view = t2d::PursuitView{f.d_rows, f.d_ctrl, f.d_target, n_ctrl, any_acc, 0};
    f.on = true;
    p->pursuit = std::move(f);
    return T2D_OK;
}

int t2d_pursuit_actions(t2d_pool* p, const float* act_in_dev, float* act_out_dev, t2d_pursuit_record* record_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    const bool no_last = p->pursuit.any_last && !(p->v.out_mask & T2D_OUT_APPLIED);
    int rc = actions_gate(p, "t2d_pursuit_actions", "t2d_set_pursuit", p->pursuit.on, p->pursuit.any_lat ? "lat_mode 1" : nullptr,
                          no_last ? "cruise / ACC read T2D_F_APPLIED0, which t2d_set_outputs switched off" : nullptr, act_out_dev,
                          record_dev);
    if (rc) return rc;
    hipStream_t s = (hipStream_t)hip_stream;
    touch(p, s);
    if ((rc = record_event(p, T2D_PROFILE_PURSUIT, s, true))) return rc;
    p->pursuit.view.episode_gate = p->applied_spans_restart ? 1 : 0;
    T2D_HIP(p, t2d::launch_pursuit(p->v, p->pursuit.view, p->route, act_in_dev, act_out_dev,
                                   record_dev ? record_dev : p->pursuit.d_rec.get(), s));
    return record_event(p, T2D_PROFILE_PURSUIT, s, false);
}

int t2d_pursuit_buffers(t2d_pool* p, void** records_dev, size_t* nbytes) {
    if (!p) return T2D_ERR_INVALID;
    return own_records(p, p->pursuit.on, "t2d_set_pursuit must precede t2d_pursuit_buffers", p->pursuit.d_rec.get(),
                       (size_t)p->v.N * sizeof(t2d_pursuit_record), records_dev, nbytes);
}

int t2d_verify_state(t2d_pool* p, const float* x_dev, const float* y_dev, const float* heading_dev,
                     const float* speed_dev, int32_t interval_ms, uint8_t* valid_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_verify_state");
    if (!x_dev || !y_dev || !heading_dev || !speed_dev || !valid_dev)
        return fail(p, T2D_ERR_INVALID, "t2d_verify_state: null device array");
    if (interval_ms < 0) return fail(p, T2D_ERR_INVALID, "interval_ms must be >= 0");
    touch(p, (hipStream_t)hip_stream);
    T2D_HIP(p, t2d::launch_verify(p->v, x_dev, y_dev, heading_dev, speed_dev, interval_ms, valid_dev,
                                  (hipStream_t)hip_stream));
    return T2D_OK;
}

// ---- device-resident trajectories (kernels: t2d_history.hip) ----------------------------------------------------------------
struct t2d_traj {
    t2d_pool* pool;
    int device, N, capacity;
    t2d::DevBuf<float> buf;   // [T2D_TRAJ_COLS][capacity][N]
    // the frame -> slot map and intervals of t2d_verify_states, staged through pinned host memory; `meta_done` follows the last
    // launch that read them, so the next call does not overwrite them under a running kernel
    int32_t meta_cap = 0;
    t2d::PinBuf<> meta_host;
    t2d::DevBuf<> meta_dev;
    hipEvent_t meta_done = nullptr;
    bool meta_pending = false;
    int n_bound = 0;   // pools that replay this trajectory (t2d_replay_bind)
};

namespace {
size_t traj_meta_bytes(int n) { return (size_t)n * sizeof(double) + (size_t)n * sizeof(int32_t); }
bool traj_slot_ok(const t2d_traj* t, int32_t slot) { return slot >= 0 && slot < t->capacity; }
}  // namespace

// a pool that goes lets go of the trajectories it replays / takes its routes from
static void unbind_trajectories(t2d_pool* p) {
    for (t2d_traj** t : {&p->replay_src, &p->route_src}) {
        if (*t) (*t)->n_bound--;
        *t = nullptr;
    }
}

int t2d_traj_create(t2d_pool* p, int32_t capacity, t2d_traj** out) {
    if (!p || !out) return p ? fail(p, T2D_ERR_INVALID, "t2d_traj_create: null output") : T2D_ERR_INVALID;
    if (capacity < 1) return fail(p, T2D_ERR_INVALID, "t2d_traj_create: capacity must be >= 1");
    T2D_HIP(p, hipSetDevice(p->device));
    std::unique_ptr<t2d_traj> t(new (std::nothrow) t2d_traj);
    if (!t) return fail(p, T2D_ERR_NOMEM, "t2d_traj_create: host allocation");
    t->pool = p;
    t->device = p->device;
    t->N = p->v.N;
    t->capacity = capacity;
    const size_t bytes = (size_t)T2D_TRAJ_COLS * capacity * t->N * sizeof(float);
    if (t->buf.alloc(bytes / sizeof(float)) != hipSuccess)
        return fail(p, T2D_ERR_NOMEM, "t2d_traj_create: " + std::to_string(bytes) + " bytes of device memory");
    if (hipEventCreateWithFlags(&t->meta_done, hipEventDisableTiming) != hipSuccess) {
        return fail(p, T2D_ERR_HIP, "t2d_traj_create: hipEventCreateWithFlags failed");
    }
    *out = t.release();
    return T2D_OK;
}

int t2d_traj_destroy(t2d_traj* t) {
    if (!t) return T2D_OK;
    if (t->n_bound > 0)
        return fail(t->pool, T2D_ERR_STATE, "t2d_traj_destroy: " + std::to_string(t->n_bound) + " pool(s) still replay this trajectory "
                                             "or take their routes from it (t2d_replay_bind with a null source / t2d_set_routes with "
                                             "n_sets = 0, or t2d_destroy of the stepped pool, first)");
    (void)hipSetDevice(t->device);
    (void)quiesce(t->pool);   // records, copies and verify launches on the pool's streams
    if (t->meta_pending) (void)hipEventSynchronize(t->meta_done);
    if (t->meta_done) (void)hipEventDestroy(t->meta_done);
    delete t;
    return T2D_OK;
}

int t2d_traj_record(t2d_traj* t, int32_t slot, void* hip_stream) {
    if (!t) return T2D_ERR_INVALID;
    t2d_pool* p = t->pool;
    if (!traj_slot_ok(t, slot)) return fail(p, T2D_ERR_INVALID, "t2d_traj_record: slot " + std::to_string(slot) + " outside [0, " +
                                                                   std::to_string(t->capacity) + ")");
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_traj_record");
    T2D_HIP(p, hipSetDevice(t->device));
    touch(p, (hipStream_t)hip_stream);
    T2D_HIP(p, t2d::launch_traj_record(p->v, t->buf, t->capacity, slot, (hipStream_t)hip_stream));
    return T2D_OK;
}

namespace {
// the six rows of one slot <-> a host block of T2D_TRAJ_COLS x N floats (one 2-D copy), after the pool's work
int traj_rows(t2d_traj* t, int32_t slot, float* host, bool to_device, const char* what) {
    t2d_pool* p = t->pool;
    if (!host) return fail(p, T2D_ERR_INVALID, std::string(what) + ": null host pointer");
    if (!traj_slot_ok(t, slot)) return fail(p, T2D_ERR_INVALID, std::string(what) + ": slot " + std::to_string(slot) + " outside [0, " +
                                                                   std::to_string(t->capacity) + ")");
    T2D_HIP(p, hipSetDevice(t->device));
    T2D_HIP(p, quiesce(p));
    const size_t row = (size_t)t->N * sizeof(float), pitch = row * t->capacity;
    float* dev = t->buf + (size_t)slot * t->N;
    if (to_device) T2D_HIP(p, hipMemcpy2D(dev, pitch, host, row, row, T2D_TRAJ_COLS, hipMemcpyHostToDevice));
    else T2D_HIP(p, hipMemcpy2D(host, row, dev, pitch, row, T2D_TRAJ_COLS, hipMemcpyDeviceToHost));
    return T2D_OK;
}
}  // namespace

int t2d_traj_write(t2d_traj* t, int32_t slot, const float* cols_host) {
    if (!t) return T2D_ERR_INVALID;
    return traj_rows(t, slot, const_cast<float*>(cols_host), true, "t2d_traj_write");
}

int t2d_traj_read(t2d_traj* t, int32_t slot, float* cols_host) {
    if (!t) return T2D_ERR_INVALID;
    return traj_rows(t, slot, cols_host, false, "t2d_traj_read");
}

int t2d_traj_column(t2d_traj* t, int32_t col, void** dev_ptr, size_t* nbytes) {
    if (!t) return T2D_ERR_INVALID;
    if (!dev_ptr || !nbytes) return fail(t->pool, T2D_ERR_INVALID, "t2d_traj_column: null output");
    if (col < 0 || col >= T2D_TRAJ_COLS) return fail(t->pool, T2D_ERR_INVALID, "t2d_traj_column: column outside [0, T2D_TRAJ_COLS)");
    const size_t n = (size_t)t->capacity * t->N;
    *dev_ptr = t->buf + (size_t)col * n;
    *nbytes = n * sizeof(float);
    return T2D_OK;
}

int t2d_traj_copy(t2d_traj* dst, const t2d_traj* src, int32_t n_slots, void* hip_stream) {
    if (!dst) return T2D_ERR_INVALID;
    t2d_pool* p = dst->pool;
    if (!src) return fail(p, T2D_ERR_INVALID, "t2d_traj_copy: null source");
    if (src->N != dst->N || src->device != dst->device)
        return fail(p, T2D_ERR_INVALID, "t2d_traj_copy: the trajectories differ in N or device");
    if (n_slots < 0 || n_slots > src->capacity || n_slots > dst->capacity)
        return fail(p, T2D_ERR_INVALID, "t2d_traj_copy: n_slots outside [0, min(capacities)]");
    if (n_slots == 0 || src == dst) return T2D_OK;
    T2D_HIP(p, hipSetDevice(dst->device));
    touch(p, (hipStream_t)hip_stream);
    if (src->pool != p) touch(src->pool, (hipStream_t)hip_stream);
    const size_t row = (size_t)dst->N * sizeof(float);
    T2D_HIP(p, hipMemcpy2DAsync(dst->buf, row * dst->capacity, src->buf, row * src->capacity, row * n_slots, T2D_TRAJ_COLS,
                                hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
    return T2D_OK;
}

int t2d_verify_states(t2d_traj* t, int32_t n_frames, const int32_t* slot_host, const double* interval_ms_host,
                      uint8_t* valid_dev, void* hip_stream) {
    if (!t) return T2D_ERR_INVALID;
    t2d_pool* p = t->pool;
    if (!slot_host || !interval_ms_host || !valid_dev) return fail(p, T2D_ERR_INVALID, "t2d_verify_states: null pointer");
    if (n_frames < 1) return fail(p, T2D_ERR_INVALID, "t2d_verify_states: n_frames must be >= 1");
    for (int k = 0; k < n_frames; ++k)
        if (!traj_slot_ok(t, slot_host[k]))
            return fail(p, T2D_ERR_INVALID, "t2d_verify_states: frame " + std::to_string(k) + " names slot " +
                                                std::to_string(slot_host[k]) + ", outside [0, " + std::to_string(t->capacity) + ")");
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_verify_states");
    int stable = 1;   // (bit equality: the ranges computed once are then those of every frame)
    for (int k = 2; k < n_frames; ++k)
        if (memcmp(&interval_ms_host[k], &interval_ms_host[1], sizeof(double)) != 0) stable = 0;
    T2D_HIP(p, hipSetDevice(t->device));
    if (t->meta_pending) {
        T2D_HIP(p, hipEventSynchronize(t->meta_done));
        t->meta_pending = false;
    }
    if (n_frames > t->meta_cap) {
        int cap = std::max(64, t->meta_cap);
        while (cap < n_frames) cap *= 2;
        t->meta_cap = 0;
        T2D_HIP(p, t->meta_dev.reset());
        T2D_HIP(p, t->meta_host.reset());
        T2D_HIP(p, t->meta_dev.alloc(traj_meta_bytes(cap)));
        T2D_HIP(p, t->meta_host.alloc(traj_meta_bytes(cap), hipHostMallocDefault));
        t->meta_cap = cap;
    }
    // [intervals: n doubles][slots: n int32] -- one copy
    memcpy(t->meta_host.get(), interval_ms_host, (size_t)n_frames * sizeof(double));
    memcpy((char*)t->meta_host.get() + (size_t)n_frames * sizeof(double), slot_host, (size_t)n_frames * sizeof(int32_t));
    const hipStream_t s = (hipStream_t)hip_stream;
    touch(p, s);
    T2D_HIP(p, hipMemcpyAsync(t->meta_dev, t->meta_host, traj_meta_bytes(n_frames), hipMemcpyHostToDevice, s));
    const double* iv_dev = (const double*)t->meta_dev.get();
    const int32_t* slot_dev = (const int32_t*)((const char*)t->meta_dev.get() + (size_t)n_frames * sizeof(double));
    T2D_HIP(p, t2d::launch_verify_states(p->v, t->buf, t->capacity, slot_dev, iv_dev, n_frames, stable, valid_dev, s));
    T2D_HIP(p, hipEventRecord(t->meta_done, s));
    t->meta_pending = true;
    return T2D_OK;
}

// ---- replayed participants (kernel: t2d_history.hip replay_kernel) --------------------------------------------------------
static void replay_release(t2d_pool* p) {
    if (p->replay_src) p->replay_src->n_bound--;
    p->replay_src = nullptr;
    p->d_replay_meta = {};
    p->replay = t2d::ReplaySpec{};
}

static int replay_impl(t2d_pool* p, int step_ms, hipStream_t s) {
    touch(p, s);
    if (p->replay_src->pool != p) touch(p->replay_src->pool, s);   // (the source pool's set-up calls wait for readers of its buffer too)
    t2d::ReplaySpec r = p->replay;
    r.type_mask = p->replay_types;
    T2D_HIP(p, t2d::launch_replay(p->v, r, step_ms, s));
    return T2D_OK;
}

int t2d_replay_bind(t2d_pool* p, const t2d_traj* src, int32_t n_slots, int32_t t0_ms, int32_t period_ms,
                    const int32_t* src_env, const int32_t* offset_ms, const int32_t* first_slot, const int32_t* last_slot) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    if (!src) {
        T2D_HIP(p, quiesce(p));
        replay_release(p);
        return T2D_OK;
    }
    const int E = p->v.n_env, A = p->v.A;
    if (src->device != p->device || src->pool->v.A != A)
        return fail(p, T2D_ERR_INVALID, "t2d_replay_bind: the source belongs to a pool of another max_agents or device");
    const int n_src_env = src->N / A, N_src = src->N;
    if (period_ms < 1) return fail(p, T2D_ERR_INVALID, "t2d_replay_bind: period_ms must be >= 1");
    if (n_slots < 1 || n_slots > src->capacity)
        return fail(p, T2D_ERR_INVALID, "t2d_replay_bind: n_slots " + std::to_string(n_slots) + " outside [1, " +
                                            std::to_string(src->capacity) + "] (the source's capacity)");
    if (t0_ms % period_ms != 0)
        return fail(p, T2D_ERR_INVALID, "t2d_replay_bind: t0_ms " + std::to_string(t0_ms) + " is not a multiple of period_ms " +
                                            std::to_string(period_ms) + " (env time starts at 0: no step could land on a stamp)");
    if (!src_env && n_src_env != E)
        return fail(p, T2D_ERR_INVALID, "t2d_replay_bind: a null src_env maps env e to source env e and needs as many source envs (" +
                                            std::to_string(n_src_env) + ") as envs (" + std::to_string(E) + ")");
    if ((first_slot == nullptr) != (last_slot == nullptr))
        return fail(p, T2D_ERR_INVALID, "t2d_replay_bind: pass both window arrays or neither");
    // [src_env | offset_ms | first_slot | last_slot], each padded to a multiple of four words (16-byte loads of the windows)
    const size_t e4 = ((size_t)E + 3) & ~(size_t)3, n4 = ((size_t)N_src + 3) & ~(size_t)3;
    std::vector<int32_t> meta(2 * e4 + 2 * n4, 0);
    int32_t *m_env = meta.data(), *m_off = m_env + e4, *m_first = m_off + e4, *m_last = m_first + n4;
    for (int e = 0; e < E; ++e) {
        m_env[e] = src_env ? src_env[e] : e;
        m_off[e] = offset_ms ? offset_ms[e] : 0;
        if (m_env[e] < 0 || m_env[e] >= n_src_env)
            return fail(p, T2D_ERR_INVALID, "t2d_replay_bind: src_env[" + std::to_string(e) + "] = " + std::to_string(m_env[e]) +
                                                " outside [0, " + std::to_string(n_src_env) + ")");
        if (m_off[e] % period_ms != 0)
            return fail(p, T2D_ERR_INVALID, "t2d_replay_bind: offset_ms[" + std::to_string(e) + "] = " + std::to_string(m_off[e]) +
                                                " is not a multiple of period_ms " + std::to_string(period_ms));
    }
    for (int j = 0; j < N_src; ++j) {
        m_first[j] = first_slot ? first_slot[j] : 0;
        m_last[j] = last_slot ? last_slot[j] : n_slots - 1;
        if (m_first[j] < 0 || m_first[j] >= n_slots || m_last[j] < 0 || m_last[j] >= n_slots)
            return fail(p, T2D_ERR_INVALID, "t2d_replay_bind: the window of source participant " + std::to_string(j) + ", [" +
                                                std::to_string(m_first[j]) + ", " + std::to_string(m_last[j]) + "], leaves [0, " +
                                                std::to_string(n_slots) + ")");
    }
    t2d::DevBuf<int32_t> d_meta;
    if (d_meta.alloc(meta.size()) != hipSuccess)
        return fail(p, T2D_ERR_NOMEM, "t2d_replay_bind: " + std::to_string(meta.size() * sizeof(int32_t)) + " bytes of device memory");
    hipError_t he = quiesce(p);   // (a step that still reads the previous binding)
    if (he == hipSuccess) he = hipMemcpy(d_meta, meta.data(), meta.size() * sizeof(int32_t), hipMemcpyHostToDevice);
    if (he != hipSuccess) return fail(p, T2D_ERR_HIP, std::string("t2d_replay_bind: ") + hipGetErrorString(he));
    replay_release(p);   // nothing can fail from here on: the new binding replaces the old one whole
    p->d_replay_meta = std::move(d_meta);
    p->replay_src = const_cast<t2d_traj*>(src);
    p->replay_src->n_bound++;
    const int32_t* m = p->d_replay_meta;
    p->replay = t2d::ReplaySpec{src->buf, m, m + e4, m + 2 * e4, m + 2 * e4 + n4, 0u,
                                src->capacity, N_src, n_slots, t0_ms, period_ms};
    return T2D_OK;
}

int t2d_replay_apply(t2d_pool* p, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_replay_apply");
    if (!p->replay_src) return fail(p, T2D_ERR_STATE, "t2d_replay_bind must precede t2d_replay_apply");
    if (!p->replay_types) return T2D_OK;   // (no row of the table is replayed: nothing to write)
    T2D_HIP(p, hipSetDevice(p->device));
    return replay_impl(p, 0, (hipStream_t)hip_stream);
}

// ---- off-route detector (kernels: t2d_route.hip) ---------------------------------------------------------------------------
static void route_release(t2d_pool* p) {
    if (p->route_src) p->route_src->n_bound--;
    p->route_src = nullptr;
    p->d_route_geo = {};
    p->route = t2d::RouteView{};
    p->route_limit.clear();
    p->route_min_limit = 0;
    p->route_n_vert = 0;
    p->route_sets_distinct = false;
}

namespace {
// route_of (NULL: `dflt(i)`) and threshold (NULL: 0) of every participant, checked against the per-env bound `limit`
int route_assignment(t2d_pool* p, const char* who, const int32_t* route_of, const float* threshold, const std::vector<int32_t>& limit,
                     bool own_index_default, std::vector<int32_t>& ro, std::vector<float>& th) {
    const int A = p->v.A, N = p->v.N;
    ro.resize(N);
    th.assign(N, 0.f);
    for (int i = 0; i < N; ++i) {
        const int e = i / A;
        ro[i] = route_of ? route_of[i] : own_index_default ? i - e * A : -1;
        if (ro[i] < -1 || ro[i] >= limit[e])
            return fail(p, T2D_ERR_INVALID, std::string(who) + ": route_of[" + std::to_string(i) + "] = " + std::to_string(ro[i]) +
                                                " outside [-1, " + std::to_string(limit[e]) + ") (env " + std::to_string(e) + ")");
        if (threshold) th[i] = threshold[i];
    }
    return T2D_OK;
}

// the pool's assignment arrays (allocated once), filled after the pool's work
int route_assignment_upload(t2d_pool* p, const std::vector<int32_t>* ro, const std::vector<float>* th) {
    const size_t N = (size_t)p->v.N;
    if (!p->d_route_of) T2D_HIP(p, p->d_route_of.alloc(N));
    if (!p->d_route_thr) T2D_HIP(p, p->d_route_thr.alloc(N));
    if (ro) T2D_HIP(p, hipMemcpy(p->d_route_of, ro->data(), N * sizeof(int32_t), hipMemcpyHostToDevice));
    if (th) T2D_HIP(p, hipMemcpy(p->d_route_thr, th->data(), N * sizeof(float), hipMemcpyHostToDevice));
    return T2D_OK;
}

// a new geometry blob of 4-byte words on the device, filled after the pool's work; the caller commits it
int route_blob(t2d_pool* p, const char* who, const std::vector<uint32_t>& words, t2d::DevBuf<>& d) {
    const size_t bytes = std::max<size_t>(words.size(), 1) * sizeof(uint32_t);
    if (d.alloc(bytes) != hipSuccess)
        return fail(p, T2D_ERR_NOMEM, std::string(who) + ": " + std::to_string(bytes) + " bytes of device memory");
    hipError_t he = quiesce(p);   // (an evaluation that still reads the previous routes)
    if (he == hipSuccess && !words.empty()) he = hipMemcpy(d, words.data(), words.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (he != hipSuccess) return fail(p, T2D_ERR_HIP, std::string(who) + ": " + hipGetErrorString(he));
    return T2D_OK;
}
}  // namespace

int t2d_set_routes(t2d_pool* p, int32_t n_sets, const int32_t* set_route_offsets, const int32_t* route_vert_offsets,
                   const float* verts_xy, const int32_t* set_of_env, const int32_t* route_of, const float* threshold) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    if (n_sets < 0) return fail(p, T2D_ERR_INVALID, "t2d_set_routes: n_sets must be >= 0");
    if (n_sets == 0 || !set_route_offsets) {
        T2D_HIP(p, quiesce(p));
        route_release(p);
        return T2D_OK;
    }
    if (!route_vert_offsets || !verts_xy) return fail(p, T2D_ERR_INVALID, "t2d_set_routes: null route_vert_offsets / verts_xy");
    const int E = p->v.n_env;
    if (set_route_offsets[0] != 0 || route_vert_offsets[0] != 0)
        return fail(p, T2D_ERR_INVALID, "t2d_set_routes: offsets must start at 0");
    for (int s = 0; s < n_sets; ++s)
        if (set_route_offsets[s + 1] < set_route_offsets[s])
            return fail(p, T2D_ERR_INVALID, "t2d_set_routes: set_route_offsets decreases at set " + std::to_string(s));
    const int n_route = set_route_offsets[n_sets];
    for (int r = 0; r < n_route; ++r)
        if (route_vert_offsets[r + 1] - (int64_t)route_vert_offsets[r] < 2)
            return fail(p, T2D_ERR_INVALID, "t2d_set_routes: route " + std::to_string(r) + " has " +
                                                std::to_string(route_vert_offsets[r + 1] - (int64_t)route_vert_offsets[r]) +
                                                " vertices (a route is a polyline of at least two; offsets must increase)");
    const int n_vert = route_vert_offsets[n_route];
    int lds_bytes = 0;
    for (int s = 0; s < n_sets; ++s) {
        const int nr = set_route_offsets[s + 1] - set_route_offsets[s];
        const int nv = route_vert_offsets[set_route_offsets[s + 1]] - route_vert_offsets[set_route_offsets[s]];
        if (nv > T2D_MAX_ROUTE_SET_VERTS)
            return fail(p, T2D_ERR_GEOMETRY, "t2d_set_routes: route set " + std::to_string(s) + " holds " + std::to_string(nv) +
                                                 " vertices, more than T2D_MAX_ROUTE_SET_VERTS = " +
                                                 std::to_string(T2D_MAX_ROUTE_SET_VERTS));
        lds_bytes = std::max(lds_bytes, nv * 8 + (nr + 1) * 4);
    }
    std::vector<int32_t> limit(E);
    for (int e = 0; e < E; ++e) {
        const int s = set_of_env ? set_of_env[e] : 0;
        if (s < 0 || s >= n_sets)
            return fail(p, T2D_ERR_INVALID, "t2d_set_routes: set_of_env[" + std::to_string(e) + "] = " + std::to_string(s) +
                                                " outside [0, " + std::to_string(n_sets) + ")");
        limit[e] = set_route_offsets[s + 1] - set_route_offsets[s];
    }
    std::vector<int32_t> ro;
    std::vector<float> th;
    int rc;
    if ((rc = route_assignment(p, "t2d_set_routes", route_of, threshold, limit, false, ro, th))) return rc;
    // [verts: 2 n_vert | set_of_env: E | set_route_start: n_sets + 1 | route_vert_off: n_route + 1]
    std::vector<uint32_t> w((size_t)2 * n_vert + E + n_sets + 1 + n_route + 1);
    memcpy(w.data(), verts_xy, (size_t)2 * n_vert * sizeof(float));
    int32_t* wi = reinterpret_cast<int32_t*>(w.data()) + (size_t)2 * n_vert;
    for (int e = 0; e < E; ++e) wi[e] = set_of_env ? set_of_env[e] : 0;
    memcpy(wi + E, set_route_offsets, (size_t)(n_sets + 1) * sizeof(int32_t));
    memcpy(wi + E + n_sets + 1, route_vert_offsets, (size_t)(n_route + 1) * sizeof(int32_t));
    t2d::DevBuf<> blob;
    if ((rc = route_blob(p, "t2d_set_routes", w, blob))) return rc;
    if ((rc = route_assignment_upload(p, &ro, &th))) return rc;
    route_release(p);   // nothing can fail from here on: the new routes replace the old ones whole
    p->d_route_geo = std::move(blob);
    const void* d = p->d_route_geo;
    p->route_limit = std::move(limit);
    p->route_n_vert = n_vert;
    p->route_min_limit = *std::min_element(p->route_limit.begin(), p->route_limit.end());
    {   // (what t2d_curve_routes asks of the installed offsets)
        std::vector<char> used(n_sets, 0);
        p->route_sets_distinct = true;
        for (int e = 0; e < E; ++e) {
            const int s = set_of_env ? set_of_env[e] : 0;
            if (used[s]) p->route_sets_distinct = false;
            used[s] = 1;
        }
    }
    t2d::RouteView& rv = p->route;
    rv.kind = 1;
    rv.lds_bytes = lds_bytes;
    rv.route_of = p->d_route_of;
    rv.threshold = p->d_route_thr;
    rv.verts = (const float*)d;
    rv.set_of_env = (const int32_t*)d + (size_t)2 * n_vert;
    rv.set_route_start = rv.set_of_env + E;
    rv.route_vert_off = rv.set_route_start + n_sets + 1;
    return T2D_OK;
}

int t2d_set_route_assignment(t2d_pool* p, const int32_t* route_of, const float* threshold) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->route.kind) return fail(p, T2D_ERR_STATE, "t2d_set_routes / t2d_set_routes_from_traj must precede t2d_set_route_assignment");
    T2D_HIP(p, hipSetDevice(p->device));
    std::vector<int32_t> ro;
    std::vector<float> th;
    int rc;
    // (checked even when only the thresholds change: a NULL route_of stands for the one installed, which was checked then)
    if (route_of && (rc = route_assignment(p, "t2d_set_route_assignment", route_of, nullptr, p->route_limit, false, ro, th))) return rc;
    if (threshold) th.assign(threshold, threshold + p->v.N);
    T2D_HIP(p, quiesce(p));
    return route_assignment_upload(p, route_of ? &ro : nullptr, threshold ? &th : nullptr);
}

int t2d_set_routes_from_traj(t2d_pool* p, const t2d_traj* src, int32_t n_slots, const int32_t* src_env, const int32_t* first_slot,
                             const int32_t* last_slot, const int32_t* route_of, const float* threshold) {
    if (!p) return T2D_ERR_INVALID;
    if (!src) return fail(p, T2D_ERR_INVALID, "t2d_set_routes_from_traj: null trajectory (t2d_set_routes(pool, 0, ...) clears the routes)");
    T2D_HIP(p, hipSetDevice(p->device));
    const int E = p->v.n_env, A = p->v.A;
    if (src->device != p->device || src->pool->v.A != A)
        return fail(p, T2D_ERR_INVALID, "t2d_set_routes_from_traj: the source belongs to a pool of another max_agents or device");
    const int n_src_env = src->N / A, N_src = src->N;
    if (n_slots < 1 || n_slots > src->capacity)
        return fail(p, T2D_ERR_INVALID, "t2d_set_routes_from_traj: n_slots " + std::to_string(n_slots) + " outside [1, " +
                                            std::to_string(src->capacity) + "] (the source's capacity)");
    if (!src_env && n_src_env != E)
        return fail(p, T2D_ERR_INVALID, "t2d_set_routes_from_traj: a null src_env maps env e to source env e and needs as many source "
                                        "envs (" + std::to_string(n_src_env) + ") as envs (" + std::to_string(E) + ")");
    if ((first_slot == nullptr) != (last_slot == nullptr))
        return fail(p, T2D_ERR_INVALID, "t2d_set_routes_from_traj: pass both window arrays or neither");
    // [src_env: E | first_slot: N_src | last_slot: N_src]
    std::vector<uint32_t> w((size_t)E + 2 * (size_t)N_src);
    int32_t *m_env = reinterpret_cast<int32_t*>(w.data()), *m_first = m_env + E, *m_last = m_first + N_src;
    for (int e = 0; e < E; ++e) {
        m_env[e] = src_env ? src_env[e] : e;
        if (m_env[e] < 0 || m_env[e] >= n_src_env)
            return fail(p, T2D_ERR_INVALID, "t2d_set_routes_from_traj: src_env[" + std::to_string(e) + "] = " + std::to_string(m_env[e]) +
                                                " outside [0, " + std::to_string(n_src_env) + ")");
    }
    for (int j = 0; j < N_src; ++j) {
        m_first[j] = first_slot ? first_slot[j] : 0;
        m_last[j] = last_slot ? last_slot[j] : n_slots - 1;
        if (m_first[j] < 0 || m_first[j] >= n_slots || m_last[j] < 0 || m_last[j] >= n_slots)
            return fail(p, T2D_ERR_INVALID, "t2d_set_routes_from_traj: the window of source participant " + std::to_string(j) + ", [" +
                                                std::to_string(m_first[j]) + ", " + std::to_string(m_last[j]) + "], leaves [0, " +
                                                std::to_string(n_slots) + ")");
    }
    std::vector<int32_t> limit(E, A), ro;
    std::vector<float> th;
    int rc;
    if ((rc = route_assignment(p, "t2d_set_routes_from_traj", route_of, threshold, limit, true, ro, th))) return rc;
    t2d::DevBuf<> blob;
    if ((rc = route_blob(p, "t2d_set_routes_from_traj", w, blob))) return rc;
    if ((rc = route_assignment_upload(p, &ro, &th))) return rc;
    route_release(p);   // nothing can fail from here on
    p->d_route_geo = std::move(blob);
    const void* d = p->d_route_geo;
    p->route_limit = std::move(limit);
    p->route_src = const_cast<t2d_traj*>(src);
    p->route_src->n_bound++;
    t2d::RouteView& rv = p->route;
    rv.kind = 2;
    rv.route_of = p->d_route_of;
    rv.threshold = p->d_route_thr;
    const size_t col = (size_t)src->capacity * N_src;
    rv.tx = src->buf;             // column 0 of [T2D_TRAJ_COLS][capacity][N_src]
    rv.ty = src->buf + col;       // column 1
    rv.src_env = (const int32_t*)d;
    rv.first_slot = rv.src_env + E;
    rv.last_slot = rv.first_slot + N_src;
    rv.N_src = N_src;
    // lanes per participant: the smallest power of two that still puts ~128 K lanes to work, at most one per segment of the
    // longest window and at most a wave (traj_verify_group_log2's rule)
    int max_segs = 0;
    for (int j = 0; j < N_src; ++j) max_segs = std::max(max_segs, m_last[j] - m_first[j]);
    int lg = 0;
    while (lg < 6 && ((int64_t)p->v.N << lg) < (1 << 17) && (1 << lg) < max_segs) ++lg;
    rv.log2_group = lg;
    return T2D_OK;
}

int t2d_off_route(t2d_pool* p, float* dist_out_dev, uint8_t* off_out_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->route.kind) return fail(p, T2D_ERR_STATE, "t2d_set_routes / t2d_set_routes_from_traj must precede t2d_off_route");
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_off_route");
    hipStream_t s = (hipStream_t)hip_stream;
    T2D_HIP(p, hipSetDevice(p->device));
    if ((!dist_out_dev || !off_out_dev) && !p->d_route_dist) {   // first use of the pool's own buffers
        t2d::DevBuf<float> dist;
        t2d::DevBuf<uint8_t> off;
        T2D_HIP(p, dist.alloc((size_t)p->v.N));
        if (off.alloc((size_t)p->v.N) != hipSuccess) return fail(p, T2D_ERR_NOMEM, "t2d_off_route: the pool's own result buffers");
        p->d_route_dist = std::move(dist);
        p->d_route_off = std::move(off);
    }
    touch(p, s);
    if (p->route_src && p->route_src->pool != p) touch(p->route_src->pool, s);   // (the source pool's set-up calls wait for readers of its buffer)
    int rc;
    if ((rc = record_event(p, 9, s, true))) return rc;
    T2D_HIP(p, t2d::launch_off_route(p->v, p->route, dist_out_dev ? dist_out_dev : p->d_route_dist,
                                     off_out_dev ? off_out_dev : p->d_route_off, s));
    return record_event(p, 9, s, false);
}

int t2d_curve_routes(t2d_pool* p, const void* words_dev, const double* start_dev, double radius, double step_size, int32_t rule,
                     int32_t route, int32_t* count_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!words_dev || !start_dev || (reinterpret_cast<uintptr_t>(words_dev) & 7u))
        return fail(p, T2D_ERR_INVALID, "t2d_curve_routes: null or misaligned words_dev / start_dev");
    if (!(radius > 0.0) || !std::isfinite(radius) || !(step_size > 0.0) || !std::isfinite(step_size))
        return fail(p, T2D_ERR_INVALID, "t2d_curve_routes: radius and step_size must be positive and finite");
    if (rule != T2D_CURVE_DUBINS && rule != T2D_CURVE_RS) return fail(p, T2D_ERR_INVALID, "t2d_curve_routes: rule must be T2D_CURVE_DUBINS or T2D_CURVE_RS");
    return write_routes(p, "t2d_curve_routes", T2D_PROFILE_CURVE_ROUTES, route, count_dev, hip_stream, [&](hipStream_t s) {
        T2D_HIP(p, t2d::launch_curve_routes(p->v, p->route, words_dev, start_dev, radius, step_size, rule, route, count_dev, s));
        return T2D_OK;
    });
}

int t2d_spline_routes(t2d_pool* p, int32_t kind, const double* ctrl_dev, const int32_t* n_ctrl_dev, int32_t max_ctrl,
                      int32_t n_interpolation, int32_t degree, const double* knots_dev, int32_t boundary_type, const double* derivs_dev,
                      int32_t route, int32_t* count_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (const char* why = t2d::spline_args_error(kind, ctrl_dev, n_ctrl_dev, max_ctrl, n_interpolation, degree, knots_dev, boundary_type,
                                                 derivs_dev))
        return fail(p, T2D_ERR_INVALID, std::string("t2d_spline_routes: ") + why);
    return write_routes(p, "t2d_spline_routes", T2D_PROFILE_SPLINE_ROUTES, route, count_dev, hip_stream, [&](hipStream_t s) {
        T2D_HIP(p, t2d::launch_spline_routes(p->v, p->route, kind, ctrl_dev, n_ctrl_dev, max_ctrl, n_interpolation, degree, knots_dev,
                                             boundary_type, derivs_dev, route, count_dev, s));
        return T2D_OK;
    });
}

int t2d_planview_routes(t2d_pool* p, const void* rec_dev, const int32_t* n_geom_dev, int32_t max_geom, int32_t rule, int32_t stride,
                        int32_t route, int32_t* count_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (const char* why = t2d::planview_args_error(rec_dev, n_geom_dev, max_geom, rule))
        return fail(p, T2D_ERR_INVALID, std::string("t2d_planview_routes: ") + why);
    if (stride < 1) return fail(p, T2D_ERR_INVALID, "t2d_planview_routes: stride must be >= 1");
    return write_routes(p, "t2d_planview_routes", T2D_PROFILE_PLANVIEW_ROUTES, route, count_dev, hip_stream, [&](hipStream_t s) {
        T2D_HIP(p, t2d::launch_planview_routes(p->v, p->route, rec_dev, n_geom_dev, max_geom, rule, stride, route, count_dev, s));
        return T2D_OK;
    });
}

int t2d_polyline_routes(t2d_pool* p, const double* points_dev, const int32_t* counts_dev, int32_t max_pts, int32_t cols, int32_t route,
                        int32_t* count_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!points_dev || !counts_dev || (reinterpret_cast<uintptr_t>(points_dev) & 7u) || (reinterpret_cast<uintptr_t>(counts_dev) & 3u))
        return fail(p, T2D_ERR_INVALID, "t2d_polyline_routes: null or misaligned points_dev (8 bytes) / counts_dev (4 bytes)");
    if (max_pts < 1 || cols < 2) return fail(p, T2D_ERR_INVALID, "t2d_polyline_routes: max_pts must be >= 1 and cols >= 2");
    return write_routes(p, "t2d_polyline_routes", T2D_PROFILE_POLYLINE_ROUTES, route, count_dev, hip_stream, [&](hipStream_t s) {
        T2D_HIP(p, t2d::launch_polyline_routes(p->v, p->route, points_dev, counts_dev, max_pts, cols, route, count_dev, s));
        return T2D_OK;
    });
}

int t2d_route_vertices(t2d_pool* p, void** verts_dev, size_t* n_vertices) {
    if (!p) return T2D_ERR_INVALID;
    if (!verts_dev || !n_vertices) return fail(p, T2D_ERR_INVALID, "null output");
    if (p->route.kind != 1) return fail(p, T2D_ERR_STATE, "t2d_route_vertices: route sets (t2d_set_routes) are not the installed kind");
    *verts_dev = const_cast<float*>(p->route.verts);
    *n_vertices = (size_t)p->route_n_vert;
    return T2D_OK;
}

int t2d_off_route_buffers(t2d_pool* p, void** dist_dev, void** off_dev, size_t* n_elements) {
    if (!p) return T2D_ERR_INVALID;
    if (!dist_dev || !off_dev || !n_elements) return fail(p, T2D_ERR_INVALID, "null output");
    if (!p->d_route_dist)
        return fail(p, T2D_ERR_STATE, "a t2d_off_route with a NULL destination must precede t2d_off_route_buffers");
    *dist_dev = p->d_route_dist;
    *off_dev = p->d_route_off;
    *n_elements = (size_t)p->v.N;
    return T2D_OK;
}

// ---- racing tile progress (kernel: t2d_track.hip) ----------------------------------------------------------------------------
static void track_release(t2d_pool* p) {
    p->d_track = {};
    p->track = t2d::TrackView{};
    p->track_n_tile.clear();
    p->trackgen = t2d::TrackGenView{};
    p->trackgen_regen = p->trackgen_used = p->trackgen_failed = false;
}

namespace {
constexpr int kTrackWords = T2D_MAX_TRACK_TILES / 32;
// byte offsets of the sections of the one allocation behind a TrackView, each on a 256-byte boundary.  The per-env state
// (visiting .. start_mask) is contiguous: t2d_track_reset / t2d_track_upload move it in one copy each way.
struct TrackLayout {
    size_t tiles, set_start, n_tile, set_of_env, visiting, num_visited, mask, status, reward, start_visiting, start_mask, bytes;
    size_t g_ncp, g_attempt, g_pose, g_line, g_bound, g_flags, g_episode, g_err;   // generated tracks only (gen_sets records)
    TrackLayout(size_t n_tile_all, size_t n_sets, size_t E, size_t gen_sets = 0) {
        size_t o = 0;
        auto take = [&](size_t b) { const size_t at = o; o += (b + 255) & ~(size_t)255; return at; };
        tiles = take(n_tile_all * 32); set_start = take((n_sets + 1) * 4); n_tile = take(n_sets * 4); set_of_env = take(E * 4);
        g_ncp = take(gen_sets * 4); g_attempt = take(gen_sets * 4); g_pose = take(gen_sets * 24); g_line = take(gen_sets * 16);
        g_bound = take(gen_sets * 16); g_flags = take(gen_sets * 4); g_episode = take(gen_sets ? E * 4 : 0); g_err = take(gen_sets ? 4 : 0);
        visiting = take(E * 4); num_visited = take(E * 4); mask = take(E * kTrackWords * 4); status = take(E * 4);
        reward = take(E * 4); start_visiting = take(E * 4); start_mask = take(E * kTrackWords * 4);
        bytes = o;
    }
};
// the view's pointers into the installed allocation `d` (which the pool's d_track owns)
void track_view_borrow(t2d::TrackView& tv, char* d, const TrackLayout& lay) {
    tv.tiles = (const float*)(d + lay.tiles);
    tv.set_start = (const int32_t*)(d + lay.set_start);
    tv.n_tile = (const int32_t*)(d + lay.n_tile);
    tv.set_of_env = (const int32_t*)(d + lay.set_of_env);
    tv.visiting = (int32_t*)(d + lay.visiting);
    tv.num_visited = (int32_t*)(d + lay.num_visited);
    tv.mask = (uint32_t*)(d + lay.mask);
    tv.status = (uint8_t*)(d + lay.status);
    tv.reward = (float*)(d + lay.reward);
    tv.start_visiting = (const int32_t*)(d + lay.start_visiting);
    tv.start_mask = (const uint32_t*)(d + lay.start_mask);
}

// the progress state of the selected envs <- (tile_visiting, mask) (null: tile 0, only tile 0 visited), in `buf` (a host image
// of the allocation); their status goes back to NORMAL, their reward to 0, and the start copy follows
void track_assign_host(char* buf, const TrackLayout& lay, int E, const uint8_t* env_mask, const int32_t* visiting, const uint32_t* mask) {
    int32_t *v = (int32_t*)(buf + lay.visiting), *nv = (int32_t*)(buf + lay.num_visited), *sv = (int32_t*)(buf + lay.start_visiting);
    uint32_t *m = (uint32_t*)(buf + lay.mask), *sm = (uint32_t*)(buf + lay.start_mask);
    uint8_t* st = (uint8_t*)(buf + lay.status);
    float* rw = (float*)(buf + lay.reward);
    for (int e = 0; e < E; ++e) {
        if (env_mask && !env_mask[e]) continue;
        uint32_t* me = m + (size_t)e * kTrackWords;
        int count = 0;
        for (int w = 0; w < kTrackWords; ++w) {
            me[w] = mask ? mask[(size_t)e * kTrackWords + w] : (w == 0 ? 1u : 0u);
            count += __builtin_popcount(me[w]);
        }
        v[e] = visiting ? visiting[e] : 0;
        nv[e] = count;
        sv[e] = v[e];
        memcpy(sm + (size_t)e * kTrackWords, me, kTrackWords * sizeof(uint32_t));
        st[4 * e] = T2D_SCENARIO_NORMAL; st[4 * e + 1] = T2D_TRAFFIC_NORMAL; st[4 * e + 2] = 0; st[4 * e + 3] = 0;
        rw[e] = 0.f;
    }
}

int track_assign(t2d_pool* p, const char* who, const uint8_t* env_mask, const int32_t* visiting, const uint32_t* mask) {
    if (!p->track.installed) return fail(p, T2D_ERR_STATE, std::string("t2d_set_tracks must precede ") + who);
    const int E = p->v.n_env;
    if (p->trackgen_regen && (visiting || mask)) {   // (regenerated tracks: the tile counts are the device's)
        T2D_HIP(p, hipSetDevice(p->device));
        T2D_HIP(p, quiesce(p));
        T2D_HIP(p, hipMemcpy(p->track_n_tile.data(), p->track.n_tile, (size_t)E * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    for (int e = 0; e < E; ++e) {
        if (env_mask && !env_mask[e]) continue;
        const int n = p->track_n_tile[e];
        if (visiting && (visiting[e] < 0 || visiting[e] >= n))
            return fail(p, T2D_ERR_INVALID, std::string(who) + ": tile_visiting[" + std::to_string(e) + "] = " + std::to_string(visiting[e]) +
                                                " outside the env's ring [0, " + std::to_string(n) + ")");
        if (mask)
            for (int w = n / 32; w < kTrackWords; ++w) {
                const uint32_t beyond = w == n / 32 ? ~((1u << (n & 31)) - 1u) : 0xffffffffu;
                if (mask[(size_t)e * kTrackWords + w] & beyond)
                    return fail(p, T2D_ERR_INVALID, std::string(who) + ": the mask of env " + std::to_string(e) + " has bits beyond its " +
                                                        std::to_string(n) + " tiles");
            }
    }
    T2D_HIP(p, hipSetDevice(p->device));
    const TrackLayout lay(0, 0, (size_t)E);   // (only differences of the state sections' offsets are used)
    const size_t bytes = lay.bytes - lay.visiting;
    std::vector<char> img(lay.bytes);
    char* dev = (char*)p->track.visiting;
    T2D_HIP(p, quiesce(p));
    T2D_HIP(p, hipMemcpy(img.data() + lay.visiting, dev, bytes, hipMemcpyDeviceToHost));
    track_assign_host(img.data(), lay, E, env_mask, visiting, mask);
    T2D_HIP(p, hipMemcpy(dev, img.data() + lay.visiting, bytes, hipMemcpyHostToDevice));
    return T2D_OK;
}
}  // namespace

int t2d_set_tracks(t2d_pool* p, int32_t n_sets, const int32_t* set_tile_offsets, const float* tiles_xy, const int32_t* set_of_env,
                   int32_t ego_index, int32_t rule, int32_t max_advance, int32_t check_off_road) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    if (n_sets < 0) return fail(p, T2D_ERR_INVALID, "t2d_set_tracks: n_sets must be >= 0");
    if (n_sets == 0 || !set_tile_offsets) {
        T2D_HIP(p, quiesce(p));
        track_release(p);
        return T2D_OK;
    }
    if (!tiles_xy) return fail(p, T2D_ERR_INVALID, "t2d_set_tracks: null tiles_xy");
    const int E = p->v.n_env;
    if (ego_index < 0 || ego_index >= p->v.A)
        return fail(p, T2D_ERR_INVALID, "t2d_set_tracks: ego_index " + std::to_string(ego_index) + " outside [0, max_agents)");
    if (rule != T2D_TRACK_RULE_REFERENCE && rule != T2D_TRACK_RULE_FORWARD)
        return fail(p, T2D_ERR_INVALID, "t2d_set_tracks: unknown rule " + std::to_string(rule));
    if (max_advance < 0) return fail(p, T2D_ERR_INVALID, "t2d_set_tracks: max_advance must be >= 0 (0 = the whole ring)");
    if (set_tile_offsets[0] != 0) return fail(p, T2D_ERR_INVALID, "t2d_set_tracks: offsets must start at 0");
    for (int s = 0; s < n_sets; ++s) {
        const int64_t n = (int64_t)set_tile_offsets[s + 1] - set_tile_offsets[s];
        if (n < 3)
            return fail(p, T2D_ERR_INVALID, "t2d_set_tracks: track " + std::to_string(s) + " has " + std::to_string(n) +
                                                " tiles (a ring needs at least three; offsets must increase)");
        if (n > T2D_MAX_TRACK_TILES)
            return fail(p, T2D_ERR_GEOMETRY, "t2d_set_tracks: track " + std::to_string(s) + " has " + std::to_string(n) +
                                                 " tiles, more than T2D_MAX_TRACK_TILES = " + std::to_string(T2D_MAX_TRACK_TILES));
    }
    const int n_tile = set_tile_offsets[n_sets];
    for (size_t k = 0; k < (size_t)n_tile * 8; ++k)
        if (!__builtin_isfinite(tiles_xy[k])) return fail(p, T2D_ERR_GEOMETRY, "t2d_set_tracks: non-finite vertex in tile " + std::to_string(k / 8));
    std::vector<int32_t> n_of_env(E);
    for (int e = 0; e < E; ++e) {
        const int s = set_of_env ? set_of_env[e] : 0;
        if (s < 0 || s >= n_sets)
            return fail(p, T2D_ERR_INVALID, "t2d_set_tracks: set_of_env[" + std::to_string(e) + "] = " + std::to_string(s) +
                                                " outside [0, " + std::to_string(n_sets) + ")");
        n_of_env[e] = set_tile_offsets[s + 1] - set_tile_offsets[s];
    }
    const TrackLayout lay((size_t)n_tile, (size_t)n_sets, (size_t)E);
    std::vector<char> img(lay.bytes);
    memcpy(img.data() + lay.tiles, tiles_xy, (size_t)n_tile * 32);
    memcpy(img.data() + lay.set_start, set_tile_offsets, (size_t)(n_sets + 1) * sizeof(int32_t));
    for (int s = 0; s < n_sets; ++s) ((int32_t*)(img.data() + lay.n_tile))[s] = set_tile_offsets[s + 1] - set_tile_offsets[s];
    for (int e = 0; e < E; ++e) ((int32_t*)(img.data() + lay.set_of_env))[e] = set_of_env ? set_of_env[e] : 0;
    track_assign_host(img.data(), lay, E, nullptr, nullptr, nullptr);
    t2d::DevBuf<> blob;
    if (blob.alloc(lay.bytes) != hipSuccess)
        return fail(p, T2D_ERR_NOMEM, "t2d_set_tracks: " + std::to_string(lay.bytes) + " bytes of device memory");
    char* const d = (char*)blob.get();
    hipError_t he = quiesce(p);   // (a progress launch that still reads the previous tracks)
    if (he == hipSuccess) he = hipMemcpy(d, img.data(), lay.bytes, hipMemcpyHostToDevice);
    if (he != hipSuccess) return fail(p, T2D_ERR_HIP, std::string("t2d_set_tracks: ") + hipGetErrorString(he));
    track_release(p);   // nothing can fail from here on
    p->d_track = std::move(blob);
    p->track_n_tile = std::move(n_of_env);
    t2d::TrackView& tv = p->track;
    tv.installed = 1; tv.ego_index = ego_index; tv.rule = rule; tv.max_advance = max_advance; tv.check_off_road = check_off_road != 0;
    track_view_borrow(tv, d, lay);
    return T2D_OK;
}

int t2d_set_tracks_generated(t2d_pool* p, int32_t n_sets, uint64_t seed, int64_t first_track, int64_t track_stride,
                             double car_length, const int32_t* set_of_env, int32_t ego_index, int32_t rule, int32_t max_advance,
                             int32_t regenerate) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    const int E = p->v.n_env;
    const std::string who = "t2d_set_tracks_generated: ";
    if (n_sets < 1 || n_sets > E) return fail(p, T2D_ERR_INVALID, who + "n_sets must be in 1 .. n_env");
    if (first_track < 0) return fail(p, T2D_ERR_INVALID, who + "first_track must be >= 0");
    if (!(car_length > 0.0)) return fail(p, T2D_ERR_INVALID, who + "car_length must be > 0");
    if (ego_index < 0 || ego_index >= p->v.A)
        return fail(p, T2D_ERR_INVALID, who + "ego_index " + std::to_string(ego_index) + " outside [0, max_agents)");
    if (rule != T2D_TRACK_RULE_REFERENCE && rule != T2D_TRACK_RULE_FORWARD) return fail(p, T2D_ERR_INVALID, who + "unknown rule " + std::to_string(rule));
    if (max_advance < 0) return fail(p, T2D_ERR_INVALID, who + "max_advance must be >= 0 (0 = the whole ring)");
    if (!set_of_env && n_sets != 1 && n_sets != E)
        return fail(p, T2D_ERR_INVALID, who + "a NULL set_of_env needs n_sets = 1 (every env on track 0) or n_sets = n_env (the identity)");
    std::vector<int32_t> soe(E);
    for (int e = 0; e < E; ++e) {
        soe[e] = set_of_env ? set_of_env[e] : (n_sets == 1 ? 0 : e);
        if (soe[e] < 0 || soe[e] >= n_sets)
            return fail(p, T2D_ERR_INVALID, who + "set_of_env[" + std::to_string(e) + "] = " + std::to_string(soe[e]) + " outside [0, " + std::to_string(n_sets) + ")");
    }
    if (regenerate) {
        bool identity = n_sets == E;
        for (int e = 0; e < E && identity; ++e) identity = soe[e] == e;
        if (!identity) return fail(p, T2D_ERR_INVALID, who + "regenerate = 1 needs a track set of its own for every env (n_sets == n_env, set_of_env the identity)");
        if (track_stride < E) return fail(p, T2D_ERR_INVALID, who + "regenerate = 1 needs track_stride >= n_env (two episodes would share a stream otherwise)");
    }
    if (!p->have_params || !p->have_reset || !p->have_snapshot)
        return fail(p, T2D_ERR_STATE, who + "t2d_set_param_table, t2d_reset and t2d_snapshot must precede it");
    if (!p->d_boundary) return fail(p, T2D_ERR_STATE, who + "the pool has no out-bound boundary array to write into (t2d_set_static_geometry with a boundary)");
    const TrackLayout lay((size_t)n_sets * T2D_MAX_TRACK_TILES, (size_t)n_sets, (size_t)E, (size_t)n_sets);
    // the host image holds everything behind the tiles: the same layout without tiles, every offset lower by lay.set_start
    const TrackLayout tail(0, (size_t)n_sets, (size_t)E, (size_t)n_sets);
    if (tail.bytes + lay.set_start != lay.bytes) return fail(p, T2D_ERR_STATE, who + "internal: the two track layouts disagree");
    std::vector<char> img(tail.bytes);
    for (int s = 0; s <= n_sets; ++s) ((int32_t*)(img.data() + tail.set_start))[s] = s * T2D_MAX_TRACK_TILES;
    memcpy(img.data() + tail.set_of_env, soe.data(), (size_t)E * sizeof(int32_t));
    track_assign_host(img.data(), tail, E, nullptr, nullptr, nullptr);
    t2d::DevBuf<> blob;
    if (blob.alloc(lay.bytes) != hipSuccess) return fail(p, T2D_ERR_NOMEM, who + std::to_string(lay.bytes) + " bytes of device memory");
    char* const d = (char*)blob.get();
    t2d::TrackGenView g{};
    g.seed = seed; g.first_track = first_track; g.track_stride = track_stride; g.car_length = car_length;
    g.tiles = (float*)(d + lay.tiles); g.n_tile = (int32_t*)(d + lay.n_tile); g.n_checkpoint = (int32_t*)(d + lay.g_ncp);
    g.attempt = (int32_t*)(d + lay.g_attempt); g.start_pose = (double*)(d + lay.g_pose); g.start_line = (float*)(d + lay.g_line);
    g.boundary = (float*)(d + lay.g_bound); g.flags = (uint32_t*)(d + lay.g_flags);
    g.status = (const uint8_t*)(d + lay.status); g.episode = (int32_t*)(d + lay.g_episode); g.err = (uint32_t*)(d + lay.g_err);
    g.env_boundary = p->d_boundary;
    for (int k = 0; k < 6; ++k) g.snap[k] = p->d_snap[k];
    g.ego_index = ego_index; g.A = p->v.A;
    std::vector<uint32_t> flags(n_sets);
    std::vector<int32_t> n_of_set(n_sets);
    hipError_t he = quiesce(p);
    if (he == hipSuccess) he = hipMemcpy(d + lay.set_start, img.data(), img.size(), hipMemcpyHostToDevice);
    if (he == hipSuccess) he = t2d::launch_trackgen(g, n_sets, 0, nullptr);
    if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
    if (he == hipSuccess) he = hipMemcpy(flags.data(), g.flags, (size_t)n_sets * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (he == hipSuccess) he = hipMemcpy(n_of_set.data(), g.n_tile, (size_t)n_sets * sizeof(int32_t), hipMemcpyDeviceToHost);
    if (he != hipSuccess) return fail(p, T2D_ERR_HIP, who + hipGetErrorString(he));
    for (int s = 0; s < n_sets; ++s)
        if (flags[s] || n_of_set[s] < 3)
            return fail(p, T2D_ERR_GEOMETRY, who + "track " + std::to_string(s) + " (stream " + std::to_string((long long)(first_track + s)) + ") came back flagged (" +
                                                 (flags[s] & T2D_TRACKGEN_CAPPED ? "no attempt succeeded" : "more tiles than T2D_MAX_TRACK_TILES") + "): nothing was installed");
    // the envs' boundary, the ego's state and snapshot, from the tracks just made (nothing of them crosses to the host)
    he = t2d::launch_track_install(p->v, g, (const int32_t*)(d + lay.set_of_env), nullptr);
    if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
    if (he != hipSuccess) return fail(p, T2D_ERR_HIP, who + hipGetErrorString(he));
    track_release(p);   // nothing can fail from here on
    p->d_track = std::move(blob);
    p->track_n_tile.resize(E);
    for (int e = 0; e < E; ++e) p->track_n_tile[e] = n_of_set[soe[e]];
    p->trackgen = g;
    p->trackgen_sets = n_sets;
    p->trackgen_regen = regenerate != 0;
    t2d::TrackView& tv = p->track;
    tv.installed = 1; tv.ego_index = ego_index; tv.rule = rule; tv.max_advance = max_advance; tv.check_off_road = 0;
    track_view_borrow(tv, d, lay);
    return T2D_OK;
}

int t2d_tracks_regenerate(t2d_pool* p, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->track.installed || !p->trackgen.tiles || !p->trackgen_regen)
        return fail(p, T2D_ERR_STATE, "t2d_set_tracks_generated with regenerate = 1 must precede t2d_tracks_regenerate");
    // (the launch writes through pointers taken at the install: a boundary array or a snapshot made anew since is not theirs)
    bool same = p->trackgen.env_boundary == p->d_boundary && p->have_snapshot;
    for (int k = 0; k < 6; ++k) same = same && p->trackgen.snap[k] == p->d_snap[k];
    if (!same)
        return fail(p, T2D_ERR_STATE, "t2d_tracks_regenerate: the pool's boundary array or snapshot was replaced since "
                                      "t2d_set_tracks_generated -- install the tracks again");
    hipStream_t s = (hipStream_t)hip_stream;
    T2D_HIP(p, hipSetDevice(p->device));
    touch(p, s);
    int rc;
    if ((rc = record_event(p, T2D_PROFILE_TRACKGEN, s, true))) return rc;
    T2D_HIP(p, t2d::launch_trackgen(p->trackgen, p->v.n_env, 2, s));
    p->trackgen_used = true;
    return record_event(p, T2D_PROFILE_TRACKGEN, s, false);
}

int t2d_generated_track_buffers(t2d_pool* p, void** tiles_dev, void** n_tile_dev, void** n_checkpoint_dev, void** attempt_dev,
                                void** start_pose_dev, void** start_line_dev, void** boundary_dev, void** episode_dev,
                                size_t* n_sets) {
    if (!p) return T2D_ERR_INVALID;
    if (!tiles_dev || !n_tile_dev || !n_checkpoint_dev || !attempt_dev || !start_pose_dev || !start_line_dev || !boundary_dev ||
        !episode_dev || !n_sets)
        return fail(p, T2D_ERR_INVALID, "null output");
    if (!p->track.installed || !p->trackgen.tiles)
        return fail(p, T2D_ERR_STATE, "t2d_set_tracks_generated must precede t2d_generated_track_buffers");
    const t2d::TrackGenView& g = p->trackgen;
    *tiles_dev = g.tiles; *n_tile_dev = g.n_tile; *n_checkpoint_dev = g.n_checkpoint; *attempt_dev = g.attempt;
    *start_pose_dev = g.start_pose; *start_line_dev = g.start_line; *boundary_dev = g.boundary; *episode_dev = g.episode;
    *n_sets = (size_t)p->trackgen_sets;
    return T2D_OK;
}

int t2d_track_reset(t2d_pool* p, const uint8_t* env_mask) {
    if (!p) return T2D_ERR_INVALID;
    return track_assign(p, "t2d_track_reset", env_mask, nullptr, nullptr);
}

int t2d_track_upload(t2d_pool* p, const uint8_t* env_mask, const int32_t* tile_visiting, const uint32_t* mask) {
    if (!p) return T2D_ERR_INVALID;
    if (!tile_visiting || !mask) return fail(p, T2D_ERR_INVALID, "t2d_track_upload: null tile_visiting / mask");
    return track_assign(p, "t2d_track_upload", env_mask, tile_visiting, mask);
}

int t2d_track_progress(t2d_pool* p, int32_t write_status, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->track.installed) return fail(p, T2D_ERR_STATE, "t2d_set_tracks must precede t2d_track_progress");
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_track_progress");
    hipStream_t s = (hipStream_t)hip_stream;
    T2D_HIP(p, hipSetDevice(p->device));
    touch(p, s);
    int rc;
    if ((rc = record_event(p, 10, s, true))) return rc;
    T2D_HIP(p, t2d::launch_track_progress(p->v, p->track, write_status != 0, s));
    return record_event(p, 10, s, false);
}

int t2d_track_buffers(t2d_pool* p, void** tile_visiting_dev, void** num_visited_dev, void** mask_dev, void** status_dev,
                      void** reward_dev, size_t* n_env) {
    if (!p) return T2D_ERR_INVALID;
    if (!tile_visiting_dev || !num_visited_dev || !mask_dev || !status_dev || !reward_dev || !n_env)
        return fail(p, T2D_ERR_INVALID, "null output");
    if (!p->track.installed) return fail(p, T2D_ERR_STATE, "t2d_set_tracks must precede t2d_track_buffers");
    *tile_visiting_dev = p->track.visiting;
    *num_visited_dev = p->track.num_visited;
    *mask_dev = p->track.mask;
    *status_dev = p->track.status;
    *reward_dev = p->track.reward;
    *n_env = (size_t)p->v.n_env;
    return T2D_OK;
}

// ---- BEV camera (kernel: t2d_camera.hip) ---------------------------------------------------------------------------------------
static void camera_release(t2d_pool* p) {
    p->d_cam_class = {};
    p->d_cam_rgb = {};
    p->d_cam_geo = {};
    p->camera = t2d::CameraView{};
    p->cam_geo_gen = -1;
    p->cam_type_default = true;
}

namespace {
// the reference's resolved style of the classes (renderer/matplotlib_config.py through _resolve_style; pinned by
// tests/golden/camera_style.json)
constexpr uint8_t kCamRgb[T2D_CAMERA_N_CLASS][3] = {{255, 255, 255}, {47, 53, 66}, {178, 190, 195}, {238, 118, 110},
                                                    {43, 203, 186}, {253, 150, 68}, {69, 170, 242}, {47, 53, 66}};
constexpr uint8_t kCamZ[T2D_CAMERA_N_CLASS] = {0, 3, 5, 1, 1, 6, 1, 7};

// the camera's device copy of the caller's rings, from the host copies the lidar's edge list is made of as well: per kind
// env_poly_off [E + 1] | poly_vert_off [P + 1] | xy [V][2], one allocation, remade when the geometry has changed
int camera_refresh_geo(t2d_pool* p) {
    if (p->cam_geo_gen == p->geo_gen) return T2D_OK;
    const int E = p->v.n_env;
    size_t off[2][3], total = 0;
    bool have[2];
    auto take = [&](size_t b) { const size_t at = total; total += (b + 255) & ~(size_t)255; return at; };
    for (int k = 0; k < 2; ++k) {
        const auto& g = p->hgeo[k];
        have[k] = g.present && !p->scene_mode && (int)g.ring_env_off.size() == E + 1;
        if (!have[k]) continue;
        off[k][0] = take(g.ring_env_off.size() * 4);
        off[k][1] = take(g.ring_vert_off.size() * 4);
        off[k][2] = take(g.ring_xy.size() * 4 + 4);
    }
    t2d::DevBuf<> blob;
    if (total) {
        std::vector<char> img(total);
        for (int k = 0; k < 2; ++k) {
            if (!have[k]) continue;
            const auto& g = p->hgeo[k];
            memcpy(img.data() + off[k][0], g.ring_env_off.data(), g.ring_env_off.size() * 4);
            memcpy(img.data() + off[k][1], g.ring_vert_off.data(), g.ring_vert_off.size() * 4);
            if (!g.ring_xy.empty()) memcpy(img.data() + off[k][2], g.ring_xy.data(), g.ring_xy.size() * 4);
        }
        if (blob.alloc(total) != hipSuccess)
            return fail(p, T2D_ERR_NOMEM, "t2d_camera_render: " + std::to_string(total) + " bytes of device memory for the rings");
        hipError_t he = quiesce(p);   // (a render that still reads the previous copy)
        if (he == hipSuccess) he = hipMemcpy(blob, img.data(), total, hipMemcpyHostToDevice);
        if (he != hipSuccess) return fail(p, T2D_ERR_HIP, std::string("t2d_camera_render: ") + hipGetErrorString(he));
    } else {
        T2D_HIP(p, quiesce(p));
    }
    p->d_cam_geo = std::move(blob);
    const char* d = (const char*)p->d_cam_geo.get();
    for (int k = 0; k < 2; ++k) {
        p->camera.env_poly_off[k] = have[k] ? (const int32_t*)(d + off[k][0]) : nullptr;
        p->camera.poly_vert_off[k] = have[k] ? (const int32_t*)(d + off[k][1]) : nullptr;
        p->camera.poly_xy[k] = have[k] ? (const float*)(d + off[k][2]) : nullptr;
    }
    p->cam_geo_gen = p->geo_gen;
    return T2D_OK;
}
}  // namespace

int t2d_camera_config(t2d_pool* p, int32_t width, int32_t height, float left, float right, float front, float back,
                      int32_t bind_slot, int32_t heading_up, uint32_t layers, uint32_t format) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    if (width == 0) {
        T2D_HIP(p, quiesce(p));
        camera_release(p);
        return T2D_OK;
    }
    if (width < 1 || width > T2D_CAMERA_MAX_SIDE || height < 1 || height > T2D_CAMERA_MAX_SIDE)
        return fail(p, T2D_ERR_INVALID, "t2d_camera_config: width and height must be in 1 .. " + std::to_string(T2D_CAMERA_MAX_SIDE));
    if (!__builtin_isfinite(left) || !__builtin_isfinite(right) || !__builtin_isfinite(front) || !__builtin_isfinite(back) ||
        !(left + right > 0.f) || !(front + back > 0.f))
        return fail(p, T2D_ERR_INVALID, "t2d_camera_config: the perception range must be finite with left + right > 0 and front + back > 0");
    if (bind_slot < 0 || bind_slot >= p->v.A)
        return fail(p, T2D_ERR_INVALID, "t2d_camera_config: bind_slot " + std::to_string(bind_slot) + " outside [0, max_agents)");
    if (layers == 0 || (layers & ~(uint32_t)T2D_CAMERA_LAYER_ALL)) return fail(p, T2D_ERR_INVALID, "t2d_camera_config: unknown layer bit, or no layer");
    const uint32_t fmt = format & ~(uint32_t)T2D_CAMERA_FORMAT_NAIVE;
    if (fmt == 0 || (fmt & ~(uint32_t)(T2D_CAMERA_FORMAT_CLASS | T2D_CAMERA_FORMAT_RGB)))
        return fail(p, T2D_ERR_INVALID, "t2d_camera_config: format must be T2D_CAMERA_FORMAT_CLASS, _RGB or both");
    const size_t px = (size_t)width * height, blocks = (size_t)((width + 63) / 64) * ((height + 15) / 16);
    if (px * p->v.n_env * 3 > ((size_t)1 << 36) || blocks * p->v.n_env > 0x7fffffffull)
        return fail(p, T2D_ERR_INVALID, "t2d_camera_config: images too large for this pool");
    t2d::DevBuf<uint8_t> dc, dr;
    if ((fmt & T2D_CAMERA_FORMAT_CLASS) && dc.alloc(px * p->v.n_env) != hipSuccess)
        return fail(p, T2D_ERR_NOMEM, "t2d_camera_config: " + std::to_string(px * p->v.n_env) + " bytes of device memory");
    if ((fmt & T2D_CAMERA_FORMAT_RGB) && dr.alloc(3 * px * p->v.n_env) != hipSuccess)
        return fail(p, T2D_ERR_NOMEM, "t2d_camera_config: " + std::to_string(3 * px * p->v.n_env) + " bytes of device memory");
    const hipError_t he = quiesce(p);   // (a render into the previous images)
    if (he != hipSuccess) return fail(p, T2D_ERR_HIP, std::string("t2d_camera_config: ") + hipGetErrorString(he));
    t2d::CameraView& cv = p->camera;
    const bool fresh = !cv.configured;
    p->d_cam_class = std::move(dc);
    p->d_cam_rgb = std::move(dr);
    // the window: _calculate_bounds, then auto_scale widens the short side about the centre (matplotlib_renderer.py:137-232),
    // here as offsets from the sensor
    double x0 = -(double)left, x1 = (double)right, y0 = -(double)back, y1 = (double)front;
    const double ww = x1 - x0, wh = y1 - y0, cx = (x0 + x1) / 2, cy = (y0 + y1) / 2;
    const double res_aspect = (double)height / (double)width;
    double nw, nh;
    if (wh / ww > res_aspect) { nw = wh / res_aspect; nh = wh; }
    else { nw = ww; nh = ww * res_aspect; }
    x0 = cx - nw / 2; y1 = cy + nh / 2;
    cv.configured = 1; cv.width = width; cv.height = height; cv.bind_slot = bind_slot; cv.heading_up = heading_up != 0;
    cv.layers = layers; cv.format = format;
    cv.ux0 = (float)x0; cv.uy1 = (float)y1; cv.px_w = (float)(nw / width); cv.px_h = (float)(nh / height);
    if (fresh) {   // (a camera that is configured again keeps its palette and style)
        for (int c = 0; c < T2D_CAMERA_N_CLASS; ++c) {
            cv.palette[c] = (uint32_t)kCamRgb[c][0] | (uint32_t)kCamRgb[c][1] << 8 | (uint32_t)kCamRgb[c][2] << 16;
            cv.z_of_class[c] = kCamZ[c];
        }
        p->cam_type_default = true;
    }
    return T2D_OK;
}

int t2d_camera_set_palette(t2d_pool* p, const uint8_t* rgb, int32_t n_class) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->camera.configured) return fail(p, T2D_ERR_STATE, "t2d_camera_config must precede t2d_camera_set_palette");
    if (!rgb || n_class < 1 || n_class > T2D_CAMERA_N_CLASS)
        return fail(p, T2D_ERR_INVALID, "t2d_camera_set_palette: null rgb, or n_class outside 1 .. T2D_CAMERA_N_CLASS");
    for (int c = 0; c < n_class; ++c)
        p->camera.palette[c] = (uint32_t)rgb[3 * c] | (uint32_t)rgb[3 * c + 1] << 8 | (uint32_t)rgb[3 * c + 2] << 16;
    return T2D_OK;
}

int t2d_camera_set_style(t2d_pool* p, const uint8_t* class_of_type, const uint8_t* z_of_class) {
    if (!p) return T2D_ERR_INVALID;
    if (!p->camera.configured) return fail(p, T2D_ERR_STATE, "t2d_camera_config must precede t2d_camera_set_style");
    if (class_of_type)
        for (int t = 0; t < T2D_MAX_TYPES; ++t)
            if (class_of_type[t] != T2D_CAMERA_CLASS_BACKGROUND && (class_of_type[t] < T2D_CAMERA_CLASS_VEHICLE || class_of_type[t] > T2D_CAMERA_CLASS_PEDESTRIAN))
                return fail(p, T2D_ERR_INVALID, "t2d_camera_set_style: class_of_type[" + std::to_string(t) + "] is not a participant class");
    if (z_of_class)
        for (int c = 1; c < T2D_CAMERA_N_CLASS; ++c)
            if (z_of_class[c] == 0) return fail(p, T2D_ERR_INVALID, "t2d_camera_set_style: z-orders must be in 1 .. 255");
    if (class_of_type) memcpy(p->camera.class_of_type, class_of_type, T2D_MAX_TYPES);
    p->cam_type_default = class_of_type == nullptr;
    for (int c = 1; c < T2D_CAMERA_N_CLASS; ++c) p->camera.z_of_class[c] = z_of_class ? z_of_class[c] : kCamZ[c];
    return T2D_OK;
}

int t2d_camera_render(t2d_pool* p, void* out_class_dev, void* out_rgb_dev, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    t2d::CameraView& cv = p->camera;
    if (!cv.configured) return fail(p, T2D_ERR_STATE, "t2d_camera_config must precede t2d_camera_render");
    if (!p->have_params || !p->have_reset)
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_camera_render");
    if (((uintptr_t)out_class_dev | (uintptr_t)out_rgb_dev) & 3)
        return fail(p, T2D_ERR_INVALID, "t2d_camera_render: the images must be 4-byte aligned");
    if ((cv.layers & T2D_CAMERA_LAYER_STATIC) && !p->scene_mode && !p->hgeo[0].present)
        return fail(p, T2D_ERR_STATE, "t2d_camera_render: T2D_CAMERA_LAYER_STATIC without static geometry or generated scenes");
    if ((cv.layers & T2D_CAMERA_LAYER_LANES) && !p->hgeo[1].present)
        return fail(p, T2D_ERR_STATE, "t2d_camera_render: T2D_CAMERA_LAYER_LANES without lane geometry");
    if ((cv.layers & T2D_CAMERA_LAYER_TRACKS) && !p->track.installed)
        return fail(p, T2D_ERR_STATE, "t2d_camera_render: T2D_CAMERA_LAYER_TRACKS without t2d_set_tracks");
    if ((cv.layers & T2D_CAMERA_LAYER_TARGET) && !p->have_target)
        return fail(p, T2D_ERR_STATE, "t2d_camera_render: T2D_CAMERA_LAYER_TARGET without target areas");
    hipStream_t s = (hipStream_t)hip_stream;
    T2D_HIP(p, hipSetDevice(p->device));
    int rc;
    if ((rc = camera_refresh_geo(p))) return rc;
    if (p->scene_mode) {
        cv.scene_quads = p->scene.live.quads; cv.scene_quad_id = p->scene.live.quad_id; cv.scene_n_quads = p->scene.live.n_quads;
    } else {
        cv.scene_quads = nullptr; cv.scene_quad_id = nullptr; cv.scene_n_quads = nullptr;
    }
    if (p->cam_type_default)
        for (int t = 0; t < T2D_MAX_TYPES; ++t)
            cv.class_of_type[t] = (int)p->host_params[t][T2D_P_SHAPE] == T2D_SHAPE_CIRCLE ? T2D_CAMERA_CLASS_PEDESTRIAN : T2D_CAMERA_CLASS_VEHICLE;
    uint8_t *oc = (uint8_t*)out_class_dev, *orgb = (uint8_t*)out_rgb_dev;
    if (!oc && !orgb) { oc = p->d_cam_class; orgb = p->d_cam_rgb; }
    touch(p, s);
    if ((rc = record_event(p, T2D_PROFILE_CAMERA, s, true))) return rc;
    T2D_HIP(p, t2d::launch_camera(p->v, cv, p->track, oc, orgb, (cv.format & T2D_CAMERA_FORMAT_NAIVE) != 0, s));
    return record_event(p, T2D_PROFILE_CAMERA, s, false);
}

int t2d_camera_buffers(t2d_pool* p, void** class_dev, void** rgb_dev, size_t* class_bytes, size_t* rgb_bytes) {
    if (!p) return T2D_ERR_INVALID;
    if (!class_dev || !rgb_dev || !class_bytes || !rgb_bytes) return fail(p, T2D_ERR_INVALID, "null output");
    if (!p->camera.configured) return fail(p, T2D_ERR_STATE, "t2d_camera_config must precede t2d_camera_buffers");
    const size_t px = (size_t)p->camera.width * p->camera.height * p->v.n_env;
    *class_dev = p->d_cam_class;
    *rgb_dev = p->d_cam_rgb;
    *class_bytes = p->d_cam_class ? px : 0;
    *rgb_bytes = p->d_cam_rgb ? 3 * px : 0;
    return T2D_OK;
}

// ---- occupancy grid (kernel: t2d_occupancy.hip) ---------------------------------------------------------------------------------
int t2d_occupancy_grid(t2d_pool* p, int32_t H, int32_t W, double cell_size, double origin_x, double origin_y, double inflate,
                       int32_t include_participants, int32_t exclude_slot, double free_weight, double* weight_dev, uint8_t* mask_dev,
                       int32_t* hw_dev, int32_t* status_dev, int32_t format, void* hip_stream) {
    if (!p) return T2D_ERR_INVALID;
    if (H < 1 || W < 1) return fail(p, T2D_ERR_INVALID, "t2d_occupancy_grid: H and W must be at least 1");
    if (!(cell_size >= 1e-150 && cell_size <= 1e150)) return fail(p, T2D_ERR_INVALID, "t2d_occupancy_grid: cell_size must be in 1e-150 .. 1e150");
    if (!(inflate >= 0.0 && inflate <= 1e150)) return fail(p, T2D_ERR_INVALID, "t2d_occupancy_grid: inflate must be in 0 .. 1e150");
    if (!__builtin_isfinite(origin_x) || !__builtin_isfinite(origin_y)) return fail(p, T2D_ERR_INVALID, "t2d_occupancy_grid: the origin must be finite");
    if (!(free_weight >= 0.0) || !__builtin_isfinite(free_weight))
        return fail(p, T2D_ERR_INVALID, "t2d_occupancy_grid: free_weight must be finite and not negative");
    if (exclude_slot < -1 || exclude_slot >= p->v.A)
        return fail(p, T2D_ERR_INVALID, "t2d_occupancy_grid: exclude_slot " + std::to_string(exclude_slot) + " outside -1 .. max_agents - 1");
    if (format & ~(int32_t)T2D_OCC_FORMAT_NAIVE) return fail(p, T2D_ERR_INVALID, "t2d_occupancy_grid: unknown format bit");
    if (!weight_dev && !mask_dev) return fail(p, T2D_ERR_INVALID, "t2d_occupancy_grid: weight_dev and mask_dev are both null");
    if (((uintptr_t)weight_dev & 15) || (((uintptr_t)mask_dev | (uintptr_t)hw_dev | (uintptr_t)status_dev) & 3))
        return fail(p, T2D_ERR_INVALID, "t2d_occupancy_grid: weight_dev must be 16-byte, the other pointers 4-byte aligned");
    const size_t tiles = (size_t)((W + 31) / 32) * (size_t)((H + 31) / 32);
    if (tiles * (size_t)p->v.n_env > 0x7fffffffull) return fail(p, T2D_ERR_INVALID, "t2d_occupancy_grid: grids too large for one launch");
    if (include_participants && (!p->have_params || !p->have_reset))
        return fail(p, T2D_ERR_STATE, "t2d_set_param_table and t2d_reset must precede t2d_occupancy_grid with participants");
    hipStream_t s = (hipStream_t)hip_stream;
    T2D_HIP(p, hipSetDevice(p->device));
    int rc;
    if ((rc = camera_refresh_geo(p))) return rc;   // (the rings' device copy is the camera's)
    t2d::OccView ov{};
    ov.H = H; ov.W = W; ov.include_participants = include_participants != 0; ov.exclude_slot = exclude_slot;
    ov.cell_size = cell_size; ov.origin_x = origin_x; ov.origin_y = origin_y; ov.inflate = inflate; ov.free_weight = free_weight;
    // the window's magnitude (tests/occupancy_ref.py: window_magnitude, the same operations)
    const double fx = origin_x + (double)(W - 1) * cell_size, fy = origin_y + (double)(H - 1) * cell_size;
    ov.mwin = (fmax(fmax(fabs(origin_x), fabs(fx)), fmax(fabs(origin_y), fabs(fy))) + cell_size) + inflate;
    if (p->scene_mode) {
        ov.scene_quads = p->scene.live.quads; ov.scene_quad_id = p->scene.live.quad_id; ov.scene_n_quads = p->scene.live.n_quads;
    } else {
        ov.env_poly_off = p->camera.env_poly_off[0]; ov.poly_vert_off = p->camera.poly_vert_off[0]; ov.poly_xy = p->camera.poly_xy[0];
    }
    touch(p, s);
    if ((rc = record_event(p, T2D_PROFILE_OCCUPANCY, s, true))) return rc;
    T2D_HIP(p, t2d::launch_occupancy(p->v, ov, weight_dev, mask_dev, hw_dev, status_dev, (format & T2D_OCC_FORMAT_NAIVE) != 0, s));
    return record_event(p, T2D_PROFILE_OCCUPANCY, s, false);
}

int t2d_set_outputs(t2d_pool* p, uint32_t mask) {
    if (!p) return T2D_ERR_INVALID;
    if (mask & ~T2D_OUT_ALL) return fail(p, T2D_ERR_INVALID, "unknown output bit");
    p->v.out_mask = (int32_t)mask;
    return T2D_OK;
}

int t2d_set_integrator_variant(t2d_pool* p, int32_t variant) {
    if (!p) return T2D_ERR_INVALID;
    if (variant < 0 || variant > 3) return fail(p, T2D_ERR_INVALID, "variant must be 0 (exact), 1 (fast), 2 (fast, kinematic steps iterated) or 3 (fast, resummed whatever the pool size)");
    p->integrator_variant = variant ? 1 : 0;
    p->kin_resum = variant != 2;
    p->kin_resum_forced = variant == 3;
    p->derived_interval = -1;   // (the resummation table travels with the interval's derived values)
    return T2D_OK;
}

int t2d_profile_enable(t2d_pool* p, int32_t on) {
    if (!p) return T2D_ERR_INVALID;
    T2D_HIP(p, hipSetDevice(p->device));
    if (on && !p->prof_events) {
        p->prof_events = new hipEvent_t[2 * t2d_pool::kMaxProfSteps];
        for (int i = 0; i < 2 * t2d_pool::kMaxProfSteps; ++i) T2D_HIP(p, hipEventCreate(&p->prof_events[i]));
    }
    p->profiling = on != 0;
    p->prof_count = 0;
    return T2D_OK;
}

int t2d_profile_read(t2d_pool* p, int32_t kernel_id, double* total_ms, int64_t* launches) {
    if (!p) return T2D_ERR_INVALID;
    if (!total_ms || !launches) return fail(p, T2D_ERR_INVALID, "null output");
    T2D_HIP(p, hipSetDevice(p->device));
    T2D_HIP(p, quiesce(p));
    double tot = 0.0;
    int64_t n = 0;
    for (int i = 0; i + 1 < p->prof_count; i += 2) {
        if (p->prof_kernel[i] != kernel_id) continue;
        float ms = 0.f;
        T2D_HIP(p, hipEventElapsedTime(&ms, p->prof_events[i], p->prof_events[i + 1]));
        tot += ms;
        ++n;
    }
    *total_ms = tot;
    *launches = n;
    return T2D_OK;
}

}  // extern "C"
