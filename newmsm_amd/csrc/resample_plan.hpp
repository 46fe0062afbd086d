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
    const double *row_div = nullptr;  // nNew divisors of a smoothing plan (0.0: the row is not divided), nullptr for every other method
};

// One tile of nd <= kPlanTile maps (T = float or double): data nd x nOld map-major -> out nd x nNew map-major.  tin (nOld x kPlanTile) and tout
// (nNew x kPlanTile) are scratch: the tile in vertex-major order and the result in vertex-major order.  Three launches on the context's stream.
template <typename T>
int launch_plan_tile(msm_ctx *ctx, const PlanRows &r, const T *d_data, int nd, T *d_tin, T *d_tout, T *d_out);
// the vote of msm_resample_plan_apply_labels for D rows of keys (D x nOld -> D x nNew)
int launch_plan_labels(msm_ctx *ctx, const PlanRows &r, const int32_t *d_labels, int D, int32_t unassigned, int32_t *d_out);


// ---- the rows of a smoothing plan (smooth_plan_kernels.hip): smooth_data's neighbourhoods, R/resampler.cpp:168-230, for the N vertices of sphLow
struct SmoothRows {
    const double *unit;  // 3 x N unit vectors of sphLow's vertices and ...
    const double4 *cb;   // ... a bounding ball per 64 of them (launch_smooth_prepare, kernels.hpp)
    const int *cv;       // N: the vertex of orig closest to sphLow's vertex i (launch_closest_vertex); it then indexes sphLow (:185)
    const double *excl;  // V(orig) >= N values read by sphLow's ids, or nullptr
    int N;
    double sigma, cosang;  // cos(4 asin(sigma / 2R)) from the host's libm, like the reference's (:175)
};
// d_row_len[i] = the members of row i (0: an excluded centre, or an id outside [0, N), which raises the context's status word); N values
int launch_smooth_plan_count(msm_ctx *ctx, const SmoothRows &s, int *d_row_len);
// the rows at the offsets d_row_ptr (N + 1, the lengths' prefix sums): col ascending, val = gain exp(-g^2 / 2 sigma^2) (x excl[col]); d_div[i] = the sum of
// row i's val and d_excl_out[i] (optional) = that sum over the sum of the unmasked weights, both in stored order from 0.0
int launch_smooth_plan_fill(msm_ctx *ctx, const SmoothRows &s, const int *d_row_ptr, int *d_col, double *d_val, double *d_div, double *d_excl_out);

}  // namespace msm
