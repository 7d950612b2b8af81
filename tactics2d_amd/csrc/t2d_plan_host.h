// t2d_plan_host.h -- the checks the grid planners' entry points share (t2d_grid_dijkstra, t2d_grid_astar, t2d_hybrid_astar,
// t2d_sample_plan, t2d_prm_plan) and the tail of their launches.  Every refusal names the entry point, reads no pointer and makes
// no HIP call.  Not part of the ABI.  DESIGN.md 4.27.
#pragma once
#include <cmath>
#include <string>

#include "t2d_gridplan_dev.h"
#include "t2d_host.h"

namespace t2d {
namespace host {

class PlanEntry {
  public:
    explicit PlanEntry(const char* fn) : fn_(fn) {}

    // "<entry point>: <rule>" as T2D_ERR_INVALID: the entry point's own scalar rules go through this
    int invalid(const std::string& rule) const { return fail(nullptr, T2D_ERR_INVALID, std::string(fn_) + ": " + rule); }

    // device pointers that must be there, aligned to mask + 1 bytes; `optional` ones may be NULL
    template <class... P>
    PlanEntry& required(uintptr_t mask, const P*... p) {
        bad_pointer_ = bad_pointer_ || (misaligned(p, mask) || ...);
        return *this;
    }
    template <class... P>
    PlanEntry& optional(uintptr_t mask, const P*... p) {
        bad_pointer_ = bad_pointer_ || ((p && misaligned(p, mask)) || ...);
        return *this;
    }
    PlanEntry& workspace(const void* p) {
        has_workspace_ = true;
        return required(15u, p);
    }
    int pointers() const {
        if (!bad_pointer_) return T2D_OK;
        return invalid(has_workspace_ ? "null or misaligned device pointer (the workspace: 16 bytes)" : "null or misaligned device pointer");
    }

    int cell_origin(double cell_size, double origin_x, double origin_y) const {
        if ((cell_size >= kPlanStepMin && cell_size <= kPlanStepMax) && std::fabs(origin_x) <= kPlanXYLimit &&
            std::fabs(origin_y) <= kPlanXYLimit)
            return T2D_OK;
        return invalid("cell_size must be positive (1e-150 .. 1e150), the origin finite");
    }

    // `why`: what of the kernel sets the cap
    int grid_cap(int max_cells, const char* why) const {
        if (max_cells <= T2D_GRID_MAX_CELLS) return T2D_OK;
        return fail(nullptr, T2D_ERR_GEOMETRY, std::string(fn_) + ": a grid of " + std::to_string(max_cells) +
                                                   " cells is above T2D_GRID_MAX_CELLS = " + std::to_string(T2D_GRID_MAX_CELLS) + " (" + why + ")");
    }

    // `need`: what <entry point>_workspace_bytes returns for this launch
    int workspace_bytes(int64_t have, int64_t need) const {
        if (have >= need) return T2D_OK;
        return invalid("the workspace has " + std::to_string(have) + " bytes, " + fn_ + "_workspace_bytes asks for " + std::to_string(need));
    }

    // the tail of every entry point: nothing for an empty batch, else the device, `go()` (the hipLaunchKernelGGL) and its error
    template <class Launch>
    int launch(int device_id, int n, Launch&& go) const {
        if (n == 0) return T2D_OK;
        if (hipSetDevice(device_id) != hipSuccess) return fail(nullptr, T2D_ERR_HIP, std::string(fn_) + ": hipSetDevice failed");
        go();
        const hipError_t err = hipGetLastError();
        if (err != hipSuccess) return fail(nullptr, T2D_ERR_HIP, std::string(fn_) + ": " + hipGetErrorString(err));
        return T2D_OK;
    }

  private:
    static bool misaligned(const void* p, uintptr_t mask) { return !p || (reinterpret_cast<uintptr_t>(p) & mask); }
    const char* fn_;
    bool bad_pointer_ = false, has_workspace_ = false;
};

}  // namespace host
}  // namespace t2d
