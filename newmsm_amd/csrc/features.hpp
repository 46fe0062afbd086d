// features.hpp -- launch wrappers of features_kernels.hip (device pointers only), used by features.cpp: msm_level_features, a level's
// featurespace::initialise (M/featurespace.cpp:39-86) for all data sets in one call.
#pragma once

#include "internal.hpp"

namespace msm {

// create_exclusion (R/mesh.cpp:1257-1273) of a D x V matrix in HBM: excl[i] = 1 when a feature of vertex i lies outside [lo, hi] or is NaN, else 0 --
// msm_create_exclusion's loop and comparison; lo / hi are the thresholds with EPSILON already applied by the host
int launch_create_exclusion(msm_ctx *ctx, const double *d_data, int D, int V, double lo, double hi, double *d_excl);

}  // namespace msm
