// features_kernels.hip -- the one kernel msm_level_features (features.cpp) adds to those of the resampler, the smoothing and the histogram matching:
// create_exclusion on the device, so that a data set's mask is made where its matrix already lies and never travels.
#include "features.hpp"

namespace msm {

namespace {

// one lane per vertex; the loop over the D rows reads V apart (coalesced across the lanes) and stops at the first feature outside the range.
// !(x >= lo && x <= hi): a NaN cuts, as in msm_create_exclusion.
__global__ __launch_bounds__(256) void k_create_exclusion(const double *__restrict__ data, int D, int V, double lo, double hi, double *__restrict__ excl) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V) return;
    double e = 0.0;
    for (int d = 0; d < D; ++d) {
        const double x = data[(size_t)d * V + i];
        if (!(x >= lo && x <= hi)) {
            e = 1.0;
            break;
        }
    }
    excl[i] = e;
}

}  // namespace

int launch_create_exclusion(msm_ctx *ctx, const double *d_data, int D, int V, double lo, double hi, double *d_excl) {
    if (V <= 0) return MSM_OK;
    hipLaunchKernelGGL(k_create_exclusion, dim3((unsigned)((V + 255) / 256)), dim3(256), 0, ctx->stream, d_data, D, V, lo, hi, d_excl);
    MSM_HIP(hipGetLastError());
    return MSM_OK;
}

}  // namespace msm
