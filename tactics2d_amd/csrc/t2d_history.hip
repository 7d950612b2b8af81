// t2d_history.hip -- device-resident trajectories: record the pool's state into a slot, the reference's verify_states over
// a recorded trajectory in one launch, and the other direction: replayed participants take their state out of a trajectory.
//
// Replaces (reference, tactics2d v0.1.9rc3):
//   Trajectory.add_state                participant/trajectory/trajectory.py:115-149   (one slot per time stamp)
//   PhysicsModelBase.verify_states      physics/physics_model_base.py:53-73
//   ParticipantBase._verify_trajectory  participant/element/participant_base.py:120-131
//   ParticipantBase.is_active / get_state(frame)  participant/element/participant_base.py:166-203   (replay_kernel)
//
// Buffer layout (t2d_traj): T2D_TRAJ_COLS fp32 columns, each [capacity][N] -- a slot is one contiguous row of every column, so a
// record is six coalesced row copies and a column reads as a [frames, N] tensor.
#include "t2d_verify_dev.h"

namespace t2d {

namespace {

constexpr int kBlock = 256;

// slot `slot` of the six columns <- the pool's x, y, heading, speed, vx, vy.  blockIdx.y = column; VEC4: N % 4 == 0, so every
// row starts 16-byte aligned (hipMalloc'd columns, slot * N * 4 bytes in)
template <bool VEC4>
__global__ __launch_bounds__(kBlock) void record_kernel(PoolView pv, float* buf, size_t col_stride, size_t row_off) {
    const float* src;
    switch (blockIdx.y) {
        case 0: src = pv.x; break;
        case 1: src = pv.y; break;
        case 2: src = pv.heading; break;
        case 3: src = pv.speed; break;
        case 4: src = pv.vx; break;
        default: src = pv.vy; break;
    }
    float* dst = buf + blockIdx.y * col_stride + row_off;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (VEC4) {
        if (i < pv.N / 4) reinterpret_cast<float4*>(dst)[i] = reinterpret_cast<const float4*>(src)[i];
    } else {
        if (i < pv.N) dst[i] = src[i];
    }
}

// record_kernel in the other direction (T2D_MODEL_REPLAY, include/t2d.h): participant i of env e, when its type row has model 5,
// becomes source participant j = src_env[e] * A + agent at slot k = (frame_ms[e] + step_ms + offset_ms[e] - t0_ms) / period_ms
// where the recording has it (first_slot[j] <= k <= last_slot[j], k < n_slots): six words copied, the ids word set to
// {model 5, its type, active}; elsewhere only the active byte of the ids word is cleared.  Lanes of other types return after
// the ids load.  VEC4 (A % 4 == 0, so N, N_src and every row start are multiples of four words and a lane's four participants
// share an env): one lane takes four consecutive participants with 16-byte loads and stores -- whole vectors where the
// recording has all four, element stores where it has some.  Every load of a lane is issued before its first store.
// The per-env words (frame, source env, offset) are wave-uniform where A is a multiple of 64 and one cache line otherwise.
struct ReplayArgs {
    const float* src;            // the source trajectory's columns, each [capacity][N_src]
    size_t col_stride;           // capacity * N_src
    const int32_t* src_env;      // [n_env]
    const int32_t* offset_ms;    // [n_env]
    const int32_t* first_slot;   // [N_src]
    const int32_t* last_slot;    // [N_src]
    uint32_t type_mask;          // bit t: row t of the parameter table has model T2D_MODEL_REPLAY
    int32_t N_src, n_slots, t0_ms, period_ms, step_ms;
};

__device__ __forceinline__ bool replay_type(uint32_t ids, uint32_t type_mask) {
    const uint32_t type = (ids >> kIdsTypeShift) & 0xffu;
    return type < 32u && ((type_mask >> type) & 1u);
}
__device__ __forceinline__ uint32_t replay_ids(uint32_t ids, bool present) {
    const uint32_t type = ids & (0xffu << kIdsTypeShift);
    return present ? ((uint32_t)T2D_MODEL_REPLAY << kIdsModelShift) | type | (1u << kIdsActiveShift)
                   : ids & ~(0xffu << kIdsActiveShift);
}

template <bool VEC4>
__global__ __launch_bounds__(kBlock) void replay_kernel(PoolView pv, ReplayArgs a) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    const int g = blockIdx.x * kBlock + threadIdx.x;
    const int i = VEC4 ? 4 * g : g;   // the lane's (first) participant
    if (i >= pv.N) return;
    float* const dst[T2D_TRAJ_COLS] = {pv.x, pv.y, pv.heading, pv.speed, pv.vx, pv.vy};
    const int e = i / pv.A;
    if constexpr (VEC4) {
        const u32x4 ids = reinterpret_cast<const u32x4*>(pv.ids)[g];
        uint32_t mine = 0u;   // bit q: participant i + q is a replayed one
#pragma unroll
        for (int q = 0; q < 4; ++q) mine |= (replay_type(ids[q], a.type_mask) ? 1u : 0u) << q;
        if (mine == 0u) return;
        const int frame = pv.frame_ms[e], se = a.src_env[e], off = a.offset_ms[e];
        const int j = se * pv.A + (i - e * pv.A);
        const i32x4 first = *reinterpret_cast<const i32x4*>(a.first_slot + j), last = *reinterpret_cast<const i32x4*>(a.last_slot + j);
        const int F = frame + a.step_ms + off - a.t0_ms;
        const int k = F < 0 ? -1 : F / a.period_ms;
        uint32_t here = 0u;   // bit q: ... and the recording has it at slot k
#pragma unroll
        for (int q = 0; q < 4; ++q) here |= ((mine >> q & 1u) && k >= first[q] && k <= last[q] && k < a.n_slots ? 1u : 0u) << q;
        u32x4 nids = ids;
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (mine >> q & 1u) nids[q] = replay_ids(ids[q], here >> q & 1u);
        if (here != 0u) {   // (k is a slot of the source then: the row exists for all four)
            const float* row = a.src + (size_t)k * a.N_src + j;
            f32x4 v[T2D_TRAJ_COLS];
#pragma unroll
            for (int c = 0; c < T2D_TRAJ_COLS; ++c) v[c] = *reinterpret_cast<const f32x4*>(row + c * a.col_stride);
#pragma unroll
            for (int c = 0; c < T2D_TRAJ_COLS; ++c) {
                if (here == 15u) {
                    reinterpret_cast<f32x4*>(dst[c])[g] = v[c];
                } else {
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (here >> q & 1u) dst[c][i + q] = v[c][q];
                }
            }
        }
        if (nids[0] != ids[0] || nids[1] != ids[1] || nids[2] != ids[2] || nids[3] != ids[3])
            reinterpret_cast<u32x4*>(pv.ids)[g] = nids;
    } else {
        const uint32_t ids = pv.ids[i];
        if (!replay_type(ids, a.type_mask)) return;
        const int frame = pv.frame_ms[e], se = a.src_env[e], off = a.offset_ms[e];
        const int j = se * pv.A + (i - e * pv.A);
        const int first = a.first_slot[j], last = a.last_slot[j];
        const int F = frame + a.step_ms + off - a.t0_ms;
        const int k = F < 0 ? -1 : F / a.period_ms;
        const bool here = k >= first && k <= last && k < a.n_slots;
        if (here) {
            const float* row = a.src + (size_t)k * a.N_src + j;
            float v[T2D_TRAJ_COLS];
#pragma unroll
            for (int c = 0; c < T2D_TRAJ_COLS; ++c) v[c] = row[c * a.col_stride];
#pragma unroll
            for (int c = 0; c < T2D_TRAJ_COLS; ++c) dst[c][i] = v[c];
        }
        const uint32_t nids = replay_ids(ids, here);
        if (nids != ids) pv.ids[i] = nids;
    }
}

// verify_states: participant i is valid when every frame k in [1, n_frames) passes the check against frame 0 with interval
// interval[k] (physics_model_base.py:63-71: last_state is never advanced).  G consecutive lanes share one participant and take
// frames 1 + r, 1 + r + G, ... (r = lane in the group); the group's verdict is the AND of its lanes: a ballot for G <= 64, the
// waves' ballots through LDS for G = 128 / 256.  G = 1 at 262 144 participants (coalesced row reads, one lane each), up to 256
// for a single long trajectory.  stable: every interval[k >= 1] is the same double -- the reachable ranges are computed once.
struct VerifyStatesArgs {
    const float* buf;   // the trajectory's columns
    size_t col_stride;  // capacity * N
    const int32_t* slot;        // [n_frames] slot of frame k
    const double* interval_ms;  // [n_frames] (entry 0 unused)
    uint8_t* valid;             // [N]
    int32_t n_frames, log2_group, stable;
};

__global__ __launch_bounds__(kBlock) void verify_states_kernel(PoolView pv, VerifyStatesArgs a) {
    const int G = 1 << a.log2_group;
    const int r = threadIdx.x & (G - 1);
    const int i = blockIdx.x * (kBlock >> a.log2_group) + (threadIdx.x >> a.log2_group);
    const bool live = i < pv.N;
    bool ok = true;
    if (live) {
        const uint32_t ids = pv.ids[i];
        if ((ids >> kIdsActiveShift) & 0xffu) {
            const int type = (ids >> kIdsTypeShift) & 0xff;
            const int model = (ids >> kIdsModelShift) & 0xff;
            const size_t N = (size_t)pv.N, cs = a.col_stride;
            const float* f0 = a.buf + (size_t)a.slot[0] * N + i;
            const double lx = f0[0], ly = f0[cs], lh = f0[2 * cs], lv = f0[3 * cs], lvx = f0[4 * cs], lvy = f0[5 * cs];
            VerifyReach reach{};
            if (a.stable && 1 + r < a.n_frames) reach = verify_reach(pv.params, type, model, lx, ly, lh, lv, lvx, lvy, a.interval_ms[1]);
            for (int k = 1 + r; k < a.n_frames; k += G) {
                if (!a.stable) reach = verify_reach(pv.params, type, model, lx, ly, lh, lv, lvx, lvy, a.interval_ms[k]);
                const float* fk = a.buf + (size_t)a.slot[k] * N + i;
                if (!verify_candidate(reach, pv.params, type, fk[0], fk[cs], fk[2 * cs], fk[3 * cs])) {
                    ok = false;
                    break;
                }
            }
        }
    }
    const uint64_t bad = __ballot(!ok);
    const int lane = threadIdx.x & 63;
    if (G <= 64) {
        const uint64_t mask = (G == 64 ? ~0ull : ((1ull << G) - 1)) << (lane & ~(G - 1));
        if (live && r == 0) a.valid[i] = (bad & mask) ? 0 : 1;
        return;
    }
    __shared__ int wave_bad[kBlock / 64];
    if (lane == 0) wave_bad[threadIdx.x >> 6] = bad != 0ull;
    __syncthreads();
    if (live && r == 0) {
        int any = 0;
        for (int w = threadIdx.x >> 6; w < (int)(threadIdx.x >> 6) + (G >> 6); ++w) any |= wave_bad[w];
        a.valid[i] = any ? 0 : 1;
    }
}

}  // namespace

hipError_t launch_traj_record(const PoolView& v, float* buf, int capacity, int slot, hipStream_t s) {
    const size_t cs = (size_t)capacity * v.N, off = (size_t)slot * v.N;
    if ((v.N & 3) == 0) {
        hipLaunchKernelGGL(record_kernel<true>, dim3((v.N / 4 + kBlock - 1) / kBlock, 6), dim3(kBlock), 0, s, v, buf, cs, off);
    } else {
        hipLaunchKernelGGL(record_kernel<false>, dim3((v.N + kBlock - 1) / kBlock, 6), dim3(kBlock), 0, s, v, buf, cs, off);
    }
    return hipGetLastError();
}

hipError_t launch_replay(const PoolView& v, const ReplaySpec& r, int step_ms, hipStream_t s) {
    ReplayArgs a{r.src, (size_t)r.capacity * r.N_src, r.src_env, r.offset_ms, r.first_slot, r.last_slot, r.type_mask,
                 r.N_src, r.n_slots, r.t0_ms, r.period_ms, step_ms};
    if ((v.A & 3) == 0) {
        hipLaunchKernelGGL(replay_kernel<true>, dim3((v.N / 4 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, v, a);
    } else {
        hipLaunchKernelGGL(replay_kernel<false>, dim3((v.N + kBlock - 1) / kBlock), dim3(kBlock), 0, s, v, a);
    }
    return hipGetLastError();
}

// lanes per participant: the smallest power of two that still puts ~128 K lanes to work (two waves per SIMD), at most one per
// frame to check and at most a workgroup
int traj_verify_group_log2(int N, int n_frames) {
    int lg = 0;
    while (lg < 8 && (int64_t)N << lg < (1 << 17) && (1 << lg) < n_frames - 1) ++lg;
    return lg;
}

hipError_t launch_verify_states(const PoolView& v, const float* buf, int capacity, const int32_t* slot_dev,
                                const double* interval_dev, int n_frames, int stable, uint8_t* valid, hipStream_t s) {
    VerifyStatesArgs a{buf, (size_t)capacity * v.N, slot_dev, interval_dev, valid, n_frames, traj_verify_group_log2(v.N, n_frames),
                       stable};
    const int per_block = kBlock >> a.log2_group;
    hipLaunchKernelGGL(verify_states_kernel, dim3((v.N + per_block - 1) / per_block), dim3(kBlock), 0, s, v, a);
    return hipGetLastError();
}

}  // namespace t2d
