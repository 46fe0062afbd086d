// resample_plan.hpp -- launch wrappers of resample_plan_kernels.hip (device pointers only) and the algorithmic byte count of an apply.
#pragma once

#include "internal.hpp"

namespace msm {

// Maps per tile of an apply: a wavefront works on one output row and lane j of it on map j of the tile (tests/test_gpu_resample_plan.py
// runs D = kPlanTile - 1, kPlanTile and kPlanTile + 1).
constexpr int kPlanTile = 64;

// the rows of a plan as the kernels see them (device memory)
struct PlanRows {
    int nOld = 0, nNew = 0;
    const int *row_ptr = nullptr, *col = nullptr;
    const double *val = nullptr;
    const double *excl = nullptr;  // nOld values or nullptr
};

// One tile of nd <= kPlanTile maps (T = float or double): data nd x nOld map-major -> out nd x nNew map-major.  tin (nOld x kPlanTile) and tout
// (nNew x kPlanTile) are scratch: the tile in vertex-major order and the result in vertex-major order.  Three launches on the context's stream.
template <typename T>
int launch_plan_tile(msm_ctx *ctx, const PlanRows &r, const T *d_data, int nd, T *d_tin, T *d_tout, T *d_out);
// the vote of msm_resample_plan_apply_labels for D rows of keys (D x nOld -> D x nNew)
int launch_plan_labels(msm_ctx *ctx, const PlanRows &r, const int32_t *d_labels, int D, int32_t unassigned, int32_t *d_out);

}  // namespace msm
